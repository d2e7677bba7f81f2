"""The host build of champ_given under the host's address and undefined-behaviour sanitizers:
tools/emu/sanitize_given_main.cpp, a stand-alone program with its own main, compiled with g++ together with
tools/emu/emu_champ.cpp and run as a process of its own on the CPU.  Nothing loaded into python is sanitized, and nothing
here touches a GPU."""
import os
import subprocess

import kernel_host_build as KH

MAIN = os.path.join(KH.EMU_DIR, 'sanitize_given_main.cpp')
FLAGS = ['-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-static-libasan',
         '-static-libubsan', '-pthread', '-I' + KH.EMU_DIR]      # (the runtimes linked in: the program needs nothing preloaded)


def test_sanitized_host_build_runs_clean(tmp_path):
    exe = str(tmp_path / 'san_given')
    subprocess.check_call(['g++'] + FLAGS + [MAIN, os.path.join(KH.EMU_DIR, 'emu_champ.cpp'), '-o', exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == 'ok' and 'runtime error' not in run.stderr, (run.stdout, run.stderr)
