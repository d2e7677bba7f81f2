"""The host build of race_scenario_kernel with priors (csrc/scenario.hip.h, csrc/priors.hip.h), priors_count and the packer
of csrc/prior_pack.h under the host's address and undefined-behaviour sanitizers: tools/emu/sanitize_priors_main.cpp, a
stand-alone program with its own main, compiled with g++ together with tools/emu/emu_generic.cpp and run as a process of
its own on the CPU.  Nothing loaded into python is sanitized, and nothing here touches a GPU."""
import os
import subprocess

import kernel_host_build as KH

MAIN = os.path.join(KH.EMU_DIR, 'sanitize_priors_main.cpp')
# (the runtimes linked in: the program needs nothing preloaded; alignment: emu_generic.cpp's block of one thread puts the
# u16 `out` row and the binary32 offsets at odd LDS offsets for an odd field; a device block is a multiple of 64 threads)
FLAGS = ['-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-static-libasan',
         '-static-libubsan', '-pthread', '-fno-sanitize=alignment', '-ffp-contract=off', '-I' + KH.EMU_DIR]


def test_sanitized_host_build_runs_clean(tmp_path):
    exe = str(tmp_path / 'san_priors')
    subprocess.check_call(['g++'] + FLAGS + [MAIN, os.path.join(KH.EMU_DIR, 'emu_generic.cpp'), '-o', exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == 'ok' and 'runtime error' not in run.stderr, (run.stdout, run.stderr)
