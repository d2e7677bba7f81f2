"""The host builds of race_fastest_kernel and champ_bonus under the host's address and undefined-behaviour sanitizers:
tools/emu/sanitize_bonus_main.cpp, a stand-alone program with its own main, compiled with g++ together with
tools/emu/emu_champ.cpp or tools/emu/emu_generic.cpp and run as a process of its own on the CPU.  Nothing loaded into
python is sanitized, and nothing here touches a GPU."""
import os
import subprocess

import pytest

import kernel_host_build as KH

MAIN = os.path.join(KH.EMU_DIR, 'sanitize_bonus_main.cpp')
FLAGS = ['-std=c++17', '-g', '-O1', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-static-libasan',
         '-static-libubsan', '-pthread', '-I' + KH.EMU_DIR]      # (the runtimes linked in: the program needs nothing preloaded)
# (alignment: emu_generic.cpp's block of one thread puts the u16 `out` row at an odd LDS offset for an odd field; a
# device block is a multiple of 64 threads)
PROGRAMS = {'champ': (['-DSANITIZE_CHAMP'], 'emu_champ.cpp'),
            'fastest': (['-DSANITIZE_FASTEST', '-ffp-contract=off', '-fno-sanitize=alignment'], 'emu_generic.cpp')}


@pytest.mark.parametrize('which', sorted(PROGRAMS))
def test_sanitized_host_build_runs_clean(which, tmp_path):
    extra, driver = PROGRAMS[which]
    exe = str(tmp_path / f'san_{which}')
    subprocess.check_call(['g++'] + FLAGS + extra + [MAIN, os.path.join(KH.EMU_DIR, driver), '-o', exe])
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0 and run.stdout.strip() == 'ok' and 'runtime error' not in run.stderr, (run.stdout, run.stderr)
