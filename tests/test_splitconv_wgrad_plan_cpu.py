"""CPU: the launch plan of the split-bf16 weight gradient (arflow_amd/csrc/splitconv_wgrad_plan.hpp) walked
on the host.  tests/wgrad_plan_check.cpp includes the header the kernel includes, enumerates every block id of every launch
over N in {1, 2, 16}, C and K in {1, 31, 32, 33, 64, 65, 96, 97, 147, 563, 597}, H in {1, 4, 5, 96}, W in {1, 8, 63, 64, 65, 160}
with and without float4 staging loads, and asserts: each (chunk, output-channel tile, input-channel tile) is owned exactly
once; the workspace arflow_splitconv_wgrad_ws_bytes reports covers every store; the XCD remap is a bijection (grids of 1..17
workgroups are in the sweep, and every grid size up to 4100 is checked on its own) that gives each XCD consecutive ids.
Built with the standard library's bounds assertions; the same file builds with -fsanitize=address,undefined."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_block_of_every_launch_owns_its_tiles_once(tmp_path):
    cxx = os.environ.get('CXX') or shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    assert cxx, 'no C++ compiler on this host'
    exe = str(tmp_path / 'wgrad_plan_check')
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-D_GLIBCXX_ASSERTIONS', '-I', os.path.join(ROOT, 'arflow_amd', 'csrc'),
                            os.path.join(ROOT, 'tests', 'wgrad_plan_check.cpp'), '-o', exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith('wgrad plan ok: 17458 plans'), run.stdout
