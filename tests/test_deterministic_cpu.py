"""CPU: the deterministic-mode switch of the library -- the two new symbols, the ENONDET refusals of the
ops that only have an atomic form, the workspace size that honours the mode, and the Python context manager.  No launch
happens: everything here is argument validation or host state.  Every test leaves the mode off."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENONDET = -1004


@pytest.fixture(scope='module')
def lib():
    from arflow_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(autouse=True)
def mode_off_afterwards(lib):
    yield
    lib.arflow_set_deterministic(0)


def test_new_symbols_declared_exported_bound(lib):
    from arflow_amd import _lib
    text = open(os.path.join(ROOT, 'include', 'arflow_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in ('arflow_set_deterministic', 'arflow_get_deterministic', 'arflow_flow_up_fwd', 'arflow_flow_up_bwd'):
        assert re.search(r'\b%s\s*\(' % name, text), '%s is not declared in the header' % name
        assert hasattr(raw, name), '%s is not exported' % name
        assert name in _lib.PROTOTYPES, '%s has no ctypes prototype' % name
    assert re.search(r'#define\s+ARFLOW_ENONDET\s+\(-1004\)', text)
    assert lib.arflow_abi_version() == 10  # purely additive


def test_set_returns_previous_and_get_follows(lib):
    lib.arflow_set_deterministic(0)
    assert lib.arflow_get_deterministic() == 0
    assert lib.arflow_set_deterministic(1) == 0
    assert lib.arflow_get_deterministic() == 1
    assert lib.arflow_set_deterministic(7) == 1  # any non-zero value is "on"
    assert lib.arflow_get_deterministic() == 1
    assert lib.arflow_set_deterministic(0) == 1
    assert lib.arflow_get_deterministic() == 0


def test_initial_value_comes_from_the_environment():
    """ARFLOW_DETERMINISTIC=1 is how the mode reaches a program that does not call the API (bench.py): a fresh process
    each, no GPU touched."""
    import subprocess
    import sys
    code = 'from arflow_amd import _lib; print(_lib.load().arflow_get_deterministic())'
    for value, want in (('1', '1'), (None, '0')):
        env = dict(os.environ)
        env.pop('ARFLOW_DETERMINISTIC', None)
        if value is not None:
            env['ARFLOW_DETERMINISTIC'] = value
        out = subprocess.run([sys.executable, '-c', code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert out.stdout.strip().splitlines()[-1] == want, (value, out.stdout)


def _atomic_only_calls(lib):
    one = ctypes.c_void_p(16)
    return {
        # (gout, x1, x2, gx1, gx2, B, C, H, W, pad_size, kernel_size, max_disp, stride1, stride2, stream)
        'arflow_corr_general_bwd': lambda **k: lib.arflow_corr_general_bwd(one, one, one, one, one, k.get('B', 1), 1, 8, 8, 4, 1, 4, 1,
                                                                           1, None),
        # (gout, flow, gsrc, B, C, Hs, Ws, H, W, flow_bstride, pad, align, norm, stream)
        'arflow_warp_nearest_bwd': lambda **k: lib.arflow_warp_nearest_bwd(one, one, one, k.get('B', 1), 1, 4, 4, 4, 4, 32, 0, 1, 0,
                                                                           None),
        # (gout, src, flow, gsrc, gflow, B, C, Hs, Ws, H, W, flow_bstride, pad, align, norm, stream)
        'arflow_warp_bicubic_bwd': lambda **k: lib.arflow_warp_bicubic_bwd(one, one, one, one, None, k.get('B', 1), 1, 4, 4, 4, 4, 32,
                                                                           0, 1, 0, None),
    }


def test_ops_without_a_deterministic_form_say_so(lib):
    """With the mode on the three generic.hip scatters return ARFLOW_ENONDET from argument validation, before any launch
    (so this is safe without a GPU); an argument error still wins over it, and with the mode off the same faulty call
    returns what it returns today."""
    calls = _atomic_only_calls(lib)
    lib.arflow_set_deterministic(1)
    for name, call in calls.items():
        assert call() == ENONDET, name
        assert call(B=0) == -1002, name + ': the shape error comes first'
    lib.arflow_set_deterministic(0)
    for name, call in calls.items():
        assert call(B=0) == -1002, name
    # bicubic without gsrc (flow gradient only: a gather) and with neither gradient are not refused
    one = ctypes.c_void_p(16)
    lib.arflow_set_deterministic(1)
    assert lib.arflow_warp_bicubic_bwd(one, one, one, None, None, 1, 1, 4, 4, 4, 4, 32, 0, 1, 0, None) == 0
    assert lib.arflow_corr_general_bwd(one, one, one, None, None, 1, 1, 8, 8, 4, 1, 4, 1, 1, None) == 0
    assert b'deterministic' in lib.arflow_strerror(ENONDET)


def test_python_raises_with_deterministic_in_the_message(lib):
    from arflow_amd import _lib
    with pytest.raises(_lib.ArflowHipError, match='deterministic'):
        _lib.check(ENONDET, 'arflow_warp_nearest_bwd')


def test_workspace_size_honours_the_mode(lib):
    """The fixed-order scatter itself needs no scratch (it has no workspace-size function); the level's backward does --
    in deterministic mode it writes the gradient of the raw warped map once -- and arflow_level_bwd_ws_bytes says how much
    under the mode the call will run in."""
    B, C, H, W = 2, 32, 24, 40
    for on in (0, 1):
        lib.arflow_set_deterministic(on)
        assert lib.arflow_level_bwd_ws_bytes(0, C, H, W) == -1002
        assert lib.arflow_level_bwd_ws_bytes(B, C, -1, W) == -1002
        assert lib.arflow_level_bwd_ws_bytes(B, C, H, W) > 0
    lib.arflow_set_deterministic(0)
    off = lib.arflow_level_bwd_ws_bytes(B, C, H, W)
    lib.arflow_set_deterministic(1)
    on = lib.arflow_level_bwd_ws_bytes(B, C, H, W)
    assert on >= off + 4 * B * C * H * W
    assert on % 256 == 0


def test_flow_up_argument_errors(lib):
    one = ctypes.c_void_p(16)
    for fn in (lib.arflow_flow_up_fwd, lib.arflow_flow_up_bwd):
        assert fn(None, one, 1, 4, 4, 2, 1, None) == -1001
        assert fn(one, None, 1, 4, 4, 2, 1, None) == -1001
        assert fn(one, one, 0, 4, 4, 2, 1, None) == -1002
        assert fn(one, one, 1, 4, 0, 4, 0, None) == -1002
        assert fn(one, one, 1, 4, 4, 3, 1, None) == -1003  # factor 2 or 4


def test_context_manager_restores_after_an_exception(lib):
    from arflow_amd import functional as AF
    assert AF.is_deterministic() is False
    with pytest.raises(RuntimeError, match='boom'):
        with AF.deterministic():
            assert AF.is_deterministic() is True
            with AF.deterministic(False):
                assert AF.is_deterministic() is False
            assert AF.is_deterministic() is True
            raise RuntimeError('boom')
    assert AF.is_deterministic() is False
    assert AF.set_deterministic(True) is False
    with AF.deterministic(False):
        assert AF.is_deterministic() is False
    assert AF.is_deterministic() is True  # the PREVIOUS value, not "off"
    assert AF.set_deterministic(False) is True
