"""Pair lists of the settled mixed tiles (dense 2D P1, one order class).  The tile plan keeps for every settled tile, beside its pair codes
(tests/test_settled_tiles.py), one record with the lists the tile kernel used to build from the codes in every assembly: a header n4, n3,
n2 and the entries p | (order - 2) << 12, order 4 first, then 3, then 2, ascending pair index p within an order (pnl_device.h).  The
LISTS instantiation of k_tile_distant copies the record into LDS and takes chunk queue and order statistics from the header.  The option
PNL_SETTLED_CODES keeps the plan without lists (the kernel builds them from the codes, as before), PNL_MIXED_UNSETTLED settles nothing.

The three paths add the same local matrices in three orders: the bound is the 1e-13 max|A| that tests/test_settled_tiles.py and
test_gpu_uniform_tiles_structured_and_generic_evaluators_agree use for two summation orders of the same terms.

disc(5), 6144 cells, is the smallest disc whose plan settles tiles (1659 at s = 1/2).  The diagonal blocks of the settled tiles are
still formed pair by pair (per-point sums in the settled path are not built), so there is one settled evaluation path and
PNL_MIXED_GENERIC switches the evaluators under it as under every other path; the counter settledListTiles says which settled launch ran.
The lists are built on the device (k_tile_pair_lists), so the codes -> record check runs on the plan's own codes, on the GPU.
"""
import numpy as np
import pytest

TOL_ORDER = 1e-13           # the same terms summed in another order (tests/test_settled_tiles.py)
NOREF = 5
LIST_HEAD, LIST_STRIDE = 8, 8+4096

COUNTER_KEYS = ('numCellPairs', 'numAssembledCellPairs', 'numIntegrations', 'orders', 'singular', 'uniformTilePairs',
                'uniformTilePairsByOrder', 'workListLength')


class _options:
    """options through _lib.set_option, removed again on the way out"""

    def __init__(self, **kw):
        self.kw = {k: v for k, v in kw.items() if v is not None}

    def __enter__(self):
        from pynucleus_amd import _lib
        for k, v in self.kw.items():
            _lib.set_option(k, v)

    def __exit__(self, *exc):
        from pynucleus_amd import _lib
        for k in self.kw:
            _lib.set_option(k, None)


def _assemble(builder, **options):
    with _options(**options):
        A = builder.getDense()
        return A.toarray(), A.info['counters']


_cache = {}


def _case(s, **options):
    """builder of the disc at s and its assembly with PNL_MIXED_UNSETTLED (+ options), made once and left unchanged"""
    key = (s,)+tuple(sorted(options.items()))
    if key not in _cache:
        if ('builder', s) not in _cache:
            from pynucleus_amd import disc, PHYSICAL, P1_DoFMap, getFractionalKernel
            from pynucleus_amd.builder import nonlocalBuilder
            _cache[('builder', s)] = nonlocalBuilder(P1_DoFMap(disc(NOREF), PHYSICAL), getFractionalKernel(2, s), {'target_order': 0.5},
                                                     zeroExterior=True)
        b = _cache[('builder', s)]
        A0, cnt0 = _assemble(b, PNL_MIXED_UNSETTLED=1, **options)
        assert cnt0['settledTiles'] == 0 and cnt0['settledListTiles'] == 0
        A0.setflags(write=False)
        _cache[key] = (b, A0, cnt0)
    return _cache[key]


def _close(A, B, scale, what):
    err, derr = np.abs(A-B).max()/scale, np.abs(np.diag(A)-np.diag(B)).max()/scale
    print('%s: max|dA|/max|A| = %.3e, diagonal %.3e' % (what, err, derr))
    assert err <= TOL_ORDER and derr <= TOL_ORDER, (what, err, derr)


@pytest.mark.gpu
@pytest.mark.parametrize('s,wgs', [(0.5, None), (0.75, None), (0.4, None), (0.5, 2)])
def test_gpu_lists_codes_and_classification_agree(s, wgs):
    """s = 1/2 (KT 2), 3/4 (KT 1) and 0.4 (KT 0); with two workgroups per tile kernel one workgroup walks hundreds of settled tiles, each
    record staged inside the pipeline of the tile before.  Matrices and diagonals of the three paths agree, the statistics are equal,
    and the two settled paths take the same tiles: the default all of them with lists, PNL_SETTLED_CODES none."""
    b, A0, cnt0 = _case(s)
    AL, cntL = _assemble(b, PNL_TILE_WGS=wgs)
    AC, cntC = _assemble(b, PNL_TILE_WGS=wgs, PNL_SETTLED_CODES=1)
    print('settled tiles', cntL['settledTiles'], 'with lists', cntL['settledListTiles'])
    assert cntL['settledTiles'] > 0 and cntL['settledTiles'] == cntC['settledTiles']
    assert cntL['settledListTiles'] == cntL['settledTiles'] and cntC['settledListTiles'] == 0
    for cnt in (cntL, cntC):
        for key in COUNTER_KEYS:
            assert cnt[key] == cnt0[key], (key, cnt[key], cnt0[key])
    scale = np.abs(A0).max()
    _close(AL, A0, scale, 'lists - unsettled')
    _close(AC, A0, scale, 'codes - unsettled')
    _close(AL, AC, scale, 'lists - codes')
    assert np.abs(AL-AL.T).max() <= TOL_ORDER*scale


@pytest.mark.gpu
def test_gpu_records_restate_the_codes():
    """every settled tile: the record holds each pair with a non-zero code exactly once and no pair with code 0, grouped order 4, 3, 2
    with ascending p inside a group; the header holds the group sizes; nothing behind the last entry"""
    b, A0, cnt0 = _case(0.5)
    A1, cnt1 = _assemble(b)
    assert cnt1['settledTiles'] > 0 and cnt1['settledListTiles'] == cnt1['settledTiles']
    codes, lists = b.dense_context().settled_lists()
    n = cnt1['settledTiles']
    assert codes.shape == (n, 512) and lists is not None and lists.shape == (n, LIST_STRIDE)
    # code of pair p = 64 r + j: sweep k = r // 8 of thread (r % 8) 64 + j (tests/test_settled_tiles.py: test_code_layout_round_trips)
    p = np.arange(4096)
    r, j = p//64, p % 64
    c = (codes[:, (r % 8)*64+j].astype(np.int64) >> (2*(r//8))) & 3          # [n, 4096]: 0 none, 1 .. 3 order 2 .. 4
    want_n = np.stack([(c == 3).sum(1), (c == 2).sum(1), (c == 1).sum(1)], axis=1)
    print('pairs of order 4, 3, 2 in the settled tiles:', want_n.sum(0))
    assert (want_n.sum(0) > 0).sum() >= 2                                       # mixed tiles: more than one group is in use
    head, body = lists[:, :LIST_HEAD].astype(np.int64), lists[:, LIST_HEAD:].astype(np.int64)
    assert np.array_equal(head[:, :3], want_n) and not head[:, 3:].any()
    tot = want_n.sum(1)
    used = np.arange(4096)[None, :] < tot[:, None]
    assert not body[~used].any()
    ep, eq = body & 4095, (body >> 12)+2
    for t in range(n):
        pt, qt = ep[t, :tot[t]], eq[t, :tot[t]]
        assert np.unique(pt).shape[0] == tot[t]                                 # no pair twice
        assert np.array_equal(qt, c[t, pt]+1)                                   # its order is the code's, so no pair with code 0
        assert np.array_equal(np.sort(pt), np.flatnonzero(c[t]))                # every pair with a code
        key = (4-qt)*4096+pt
        assert (np.diff(key) > 0).all()                                         # order 4, 3, 2; ascending p inside


@pytest.mark.gpu
def test_gpu_generic_evaluators_under_the_lists():
    """PNL_MIXED_GENERIC (the evaluators for arbitrary rules): the settled launch with lists still runs, and agrees with the classifying
    path under the same option"""
    b, A0, cnt0 = _case(0.5, PNL_MIXED_GENERIC=1)
    A1, cnt1 = _assemble(b, PNL_MIXED_GENERIC=1)
    assert cnt1['settledTiles'] > 0 and cnt1['settledListTiles'] == cnt1['settledTiles']
    for key in COUNTER_KEYS:
        assert cnt1[key] == cnt0[key], (key, cnt1[key], cnt0[key])
    _close(A1, A0, np.abs(A0).max(), 'generic evaluators, lists - unsettled')


@pytest.mark.gpu
def test_gpu_option_is_part_of_the_plan_key():
    """PNL_SETTLED_CODES makes a new plan when it changes (the codes are computed again), a repeated assembly keeps the plan; a plan
    without lists hands out none"""
    b, A0, cnt0 = _case(0.5)
    A1, cnt1 = _assemble(b)
    A2, cnt2 = _assemble(b)
    assert cnt2['codeBuilds'] == cnt1['codeBuilds'] and cnt2['settledListTiles'] == cnt1['settledTiles'] > 0
    A3, cnt3 = _assemble(b, PNL_SETTLED_CODES=1)
    assert cnt3['codeBuilds'] == cnt1['codeBuilds']+1 and cnt3['settledTiles'] == cnt1['settledTiles'] and cnt3['settledListTiles'] == 0
    with _options(PNL_SETTLED_CODES=1):
        b.getDense()
        codes, lists = b.dense_context().settled_lists()
    assert lists is None and codes.shape[0] == cnt1['settledTiles']
    A4, cnt4 = _assemble(b)
    assert cnt4['codeBuilds'] == cnt3['codeBuilds']+1 and cnt4['settledListTiles'] == cnt1['settledTiles']
