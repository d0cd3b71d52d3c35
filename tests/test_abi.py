"""The C-ABI library loads and exports every symbol include/pnl_hip.h declares; host-side error paths that do
not need a GPU behave as documented.  No compute calls here (CPU-only container)."""
import ctypes
import os
import re
import numpy as np
import pytest
from pynucleus_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    txt = open(os.path.join(ROOT, 'include', 'pnl_hip.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(pnl_[a-z_0-9]+)\s*\(', txt)))


def test_header_and_binding_agree():
    assert sorted(_lib.EXPORTS) == declared_symbols()


def test_library_exports_every_declared_symbol():
    assert os.path.exists(_lib.LIB_PATH), 'build the HIP library first (__graft_entry__.build())'
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in declared_symbols():
        assert hasattr(L, name), name
    assert b'gfx950' in _lib.load().pnl_version()


def test_create_without_gpu_fails_loudly():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is visible')
    with pytest.raises(_lib.PnlError):
        _lib.Context(0)


def test_builder_has_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is visible')
    from pynucleus_amd import disc, P1_DoFMap, PHYSICAL, getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    mesh = disc(1)
    b = nonlocalBuilder(P1_DoFMap(mesh, PHYSICAL), getFractionalKernel(2, 0.5))
    with pytest.raises(_lib.PnlError):
        b.getDense()


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, 'pynucleus_amd')
    for dirpath, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith(('.py', '.hip', '.h')):
                src = open(os.path.join(dirpath, fn)).read()
                assert 'import oracle' not in src and 'from oracle' not in src and 'nl_oracle' not in src, fn


@pytest.mark.gpu
def test_work_list_overflow_fails_the_call():
    """a work list that is too small (the option PNL_WL_FRAC shrinks it to 64 entries per pass) must not pass silently: the status
    of pnl_synchronize / pnl_get_counters says the operator is incomplete (the check INTEGRATION.md's stub performs)"""
    from pynucleus_amd import disc, P1_DoFMap, P2_DoFMap, PHYSICAL, getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    from pynucleus_amd._lib import PnlError
    mesh = disc(4)
    try:
        for DoFMap in (P1_DoFMap, P2_DoFMap):
            dm = DoFMap(mesh, PHYSICAL)
            _lib.set_option('PNL_WL_FRAC', None)
            A = nonlocalBuilder(dm, getFractionalKernel(2, 0.75), {}).getDense()
            assert np.isfinite(A.toarray()).all()
            _lib.set_option('PNL_WL_FRAC', '1e-12')
            with pytest.raises(PnlError, match='work list overflow'):
                nonlocalBuilder(dm, getFractionalKernel(2, 0.75), {}).getDense()
    finally:
        _lib.set_option('PNL_WL_FRAC', None)


# the A/B switches that tuning builds of the library used to read from the environment: each was resolved to the side that had won,
# none is an option (docs/CHANGELOG_kernels.md lists them once more)
RETIRED_SWITCHES = (
    'PNL_PW_NOMIXED', 'PNL_PW_NOTILE', 'PNL_PW_NOLANE', 'PNL_ACC_PAD', 'PNL_NO_REORDER', 'PNL_ABLATE', 'PNL_WL_LANE', 'PNL_PURE',
    'PNL_NO_EXACT_TILES', 'PNL_P2_VISIT_PER_CLASS', 'PNL_UNI_QMAX', 'PNL_UNI_PER_CU', 'PNL_UNI_KEEP_STRIDE', 'PNL_UNI_ABL', 'PNL_PURE_ABL',
    'PNL_WL_DBG', 'PNL_GRID_MULT', 'PNL_PURE_V1', 'PNL_BND_PER', 'PNL_BND_DEFER', 'PNL_BT_WG', 'PNL_NO_SLOT', 'PNL_NO_KT2', 'PNL_NO_SLOT_P1',
    'PNL_BND_PER_CLASS', 'PNL_CB_PER', 'PNL_CB_DEFER', 'PNL_FORCE_SYMFLUSH', 'PNL_WL_LDS_KB', 'PNL_WL_MP_KB', 'PNL_WL_CL_KB')


def csrc_sources():
    import glob
    return {fn: open(fn).read() for fn in sorted(glob.glob(os.path.join(ROOT, 'pynucleus_amd', 'csrc', '*'))) if os.path.isfile(fn)}


def accepted_options():
    """the names of k_product_options (pnl_setup.hip), comments stripped"""
    src = open(os.path.join(ROOT, 'pynucleus_amd', 'csrc', 'pnl_setup.hip')).read()
    m = re.search(r'k_product_options\[\]\s*=\s*\{(.*?)\};', src, flags=re.S)
    assert m, 'k_product_options not found'
    body = re.sub(r'//[^\n]*', '', m.group(1))
    names = re.findall(r'"([A-Z_0-9]+)"', body)
    assert names and len(names) == len(set(names)), names
    return names


def test_option_table_matches_the_reads():
    """every option the sources read is one pnl_set_option accepts, every accepted option is read, and the name is always a literal
    at the call site (so this test sees every read)"""
    accepted = set(accepted_options())
    read = {}
    for fn, src in csrc_sources().items():
        src = re.sub(r'//[^\n]*', '', src)
        calls = re.findall(r'\bpnl_tune\s*\(\s*([^)]*)\)', src)
        for arg in calls:
            lit = re.fullmatch(r'"([A-Z_0-9]+)"\s*', arg)
            if lit:
                read.setdefault(lit.group(1), []).append(os.path.basename(fn))
            else:
                # the declaration and the definition are the only places where pnl_tune is followed by something else
                assert re.fullmatch(r'const char \*name', arg.strip()), (os.path.basename(fn), 'pnl_tune(%s)' % arg)
    assert set(read) <= accepted, sorted(set(read)-accepted)
    assert accepted <= set(read), sorted(accepted-set(read))
    assert not accepted & set(RETIRED_SWITCHES)


def test_options_are_explicit_not_environment(monkeypatch):
    """the library reads no environment variable on the assembly path: options exist only through pnl_set_option, which refuses the
    A/B switches that tuning builds used to accept; there is no such build any more"""
    L = _lib.load()
    assert b'tuning' not in L.pnl_version()
    for name in accepted_options():
        assert L.pnl_set_option(name.encode(), None) == 0, name
    for name in RETIRED_SWITCHES:
        assert L.pnl_set_option(name.encode(), b'1') == _lib.PNL_ERR_UNSUPPORTED, name
        monkeypatch.setenv(name, '1')
        assert L.pnl_set_option(name.encode(), b'1') == _lib.PNL_ERR_UNSUPPORTED, name
    assert L.pnl_set_option(b'PNL_NO_POWTAB', b'1') == 0
    assert L.pnl_set_option(b'PNL_NO_POWTAB', None) == 0
    assert L.pnl_set_option(b'PNL_NO_SLOT', b'1') == _lib.PNL_ERR_UNSUPPORTED
    with pytest.raises(_lib.PnlError):
        _lib.set_option('PNL_UNI_PER_CU', 1)
    # the planner's thread count is an option like the others
    assert L.pnl_set_option(b'PNL_PLAN_THREADS', b'2') == 0
    assert L.pnl_set_option(b'PNL_PLAN_THREADS', None) == 0
    # the staged fold and the boundary-mode switch are gone: no option selects another launch sequence, no entry point reports one
    for name in (b'PNL_FOLD_STAGES', b'PNL_UNI_SPARE', b'PNL_BND_MODE'):
        assert L.pnl_set_option(name, b'1') == _lib.PNL_ERR_UNSUPPORTED, name
    for name in ('pnl_get_fold_stages', 'pnl_get_fold_plan'):
        assert not hasattr(L, name), name
    # no getenv at all in the library sources, and nothing that a build could switch on to get one
    for fn, src in csrc_sources().items():
        assert not re.search(r'\bgetenv\b', src), fn
        assert 'PNL_TUNING' not in src and 'PNL_DEBUG_ABLATE' not in src, fn
