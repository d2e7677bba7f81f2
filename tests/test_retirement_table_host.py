"""The per-launch retirement table (csrc/params_build.h: build_retire_table) and the search in it (csrc/race_common.hip.h:
retirement_lap_from_table) as host code under the host's address and undefined-behaviour sanitizers:
tools/emu/retire_table_main.cpp, a stand-alone program with its own main, compiled with g++ and run as a process of its own
on the CPU.  The program checks, at both chain widths, that the table is the chain of draw_retirement_lap entry for entry and
that the search returns what the chain returns -- per-lap probabilities {0, 2^-32, 0.05/60, 0.01, 0.3, 0.5, 1 - 2^-32, 1},
L in {1, 2, 3, 4, 5, 60, 78, 129, 1000}, the words 0, 2^32 - 1 (2^64 - 1), every S_k - 1, S_k, S_k + 1 and 10^5 random
words each.  Nothing loaded into python is sanitized, and nothing here touches a GPU."""
import os
import subprocess

import kernel_host_build as KH

MAIN = os.path.join(KH.EMU_DIR, 'retire_table_main.cpp')
FLAGS = ['-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-static-libasan',
         '-static-libubsan', '-I' + KH.EMU_DIR]                 # (the runtimes linked in: the program needs nothing preloaded)


def test_table_is_the_chain_and_search_is_the_draw(tmp_path):
    exe = str(tmp_path / 'retire_table')
    subprocess.check_call(['g++'] + FLAGS + [MAIN, '-o', exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == 'ok' and 'runtime error' not in run.stderr, (run.stdout, run.stderr)
