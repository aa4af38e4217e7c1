"""CPU: the phase-mosaic layout of the dilated context layers (arflow_amd/csrc/phase_plan.hpp) walked on the
host.  tests/phase_plan_check.cpp includes the header the permutation kernels include and sweeps H, W in 1..70 plus 96 x 160,
384 x 640 / 4 and 384 x 640 with d in {1, 2, 4, 8, 16}: every real pixel maps to exactly one virtual element and back;
separators, ragged tails and real elements partition the virtual tensor; the chosen mosaic has the largest fill of all divisor
pairs (ties: the smaller group); d = 1 is the identity; d > H or d > W is refused; sizes stay inside the INT_MAX guards.  Built
with the standard library's bounds assertions; the same file builds and runs clean with -fsanitize=address,undefined."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_layout_is_a_bijection_on_real_pixels_and_the_mosaic_is_the_fullest(tmp_path):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler on this host'
    exe = str(tmp_path / 'phase_plan_check')
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-D_GLIBCXX_ASSERTIONS', '-I', os.path.join(ROOT, 'arflow_amd', 'csrc'),
                            os.path.join(ROOT, 'tests', 'phase_plan_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith('phase plan ok: 21159 layouts'), run.stdout
    # the flagship's mosaics (16 x 96 x 160): what DESIGN.md section 39 tabulates
    table = [line.split() for line in run.stdout.splitlines() if line.startswith('  d ')]
    got = {int(t[1]): (int(t[2]), int(t[4]), int(t[8]), int(t[10])) for t in table}
    assert got == {1: (1, 1, 96, 160), 2: (1, 1, 48, 80), 4: (1, 2, 24, 81), 8: (8, 8, 103, 167), 16: (16, 16, 111, 175)}, run.stdout
