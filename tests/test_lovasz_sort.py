"""GPU tests of the Lovász losses' segmented radix sort on its own (csrc/lovasz.hip: radix_hist_kernel,
seg_rowscan_kernel, radix_scatter_kernel through ssseg_lovasz_sort) against np.argsort(kind='stable') per segment.
Keys and values must be equal bit for bit: there is no tolerance anywhere in this file.

TILE is 2048 elements (one block of the histogram and scatter kernels) and the row scan carries 64 tiles per round,
so the lengths stand on the wave (64), tile (2048), second-round (T = 64 | 65) and third-round (T = 129) edges.
Every key family is drawn differently per segment, so a read from the neighbouring segment changes the result.  The
output sits between two runs of guard words; every case runs twice on the same (then dirty) workspace."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TILE = 2048                     # lovasz.hip: TILE = LT * ITEMS
SCAN_ROUND = 64                 # seg_rowscan_kernel: t0 += 64
MAX_S, MAX_L = 65535, 1 << 24   # ssseg_lovasz_sort's bounds (gridDim.y; fp32 counts of the losses)
GUARD = 64                      # words on each side of an output
GUARD_WORD = 0x5A5AA5A5
SENTINEL = 0xFFFFFFFF           # the key of an ignored pixel
EDGE_KEYS = np.array([0, 0x7FFFFFFF, 0x80000001, 0xFF800000, 0x80000000, 1, 0x7FFFFFFE, SENTINEL], np.uint32)

LENGTHS = [1, 63, 64, 65, 2047, 2048, 2049, 131072, 131073, 262145]
FAMILIES = ['uniform', 'equal', 'byte0', 'byte1', 'byte2', 'byte3', 'alternate', 'ascending', 'descending',
            'sentinel', 'edges']
SHAPES = [(3, 131073), (5, 4097), (65535, 3)]


def tiles(L):
    return -(-L // TILE)


def _u32(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def make_keys(family, S, L):
    """keys [S, L] uint32 of a family, each segment drawn on its own; read-only"""
    rng = np.random.default_rng([FAMILIES.index(family) if family in FAMILIES else 99, S, L])
    if family == 'uniform':
        k = _u32(rng, (S, L))
    elif family == 'equal':
        k = np.repeat(_u32(rng, (S, 1)), L, 1)
    elif family.startswith('byte'):
        sh = np.uint32(8 * int(family[4]))
        const = np.repeat(_u32(rng, (S, 1)), L, 1) & ~(np.uint32(255) << sh)
        k = const | ((_u32(rng, (S, L)) & np.uint32(255)) << sh)
    elif family == 'alternate':
        ab = _u32(rng, (S, 2))
        k = np.where((np.arange(L) & 1)[None] == 0, ab[:, :1], ab[:, 1:])
    elif family in ('ascending', 'descending'):
        k = np.sort(_u32(rng, (S, L)), 1)
        k = k[:, ::-1] if family == 'descending' else k
    elif family == 'sentinel':
        # runs of the ignored pixels' key: whole tiles, across tile edges, the first and the last elements; shifted per
        # segment so that no two segments have the same runs
        k = _u32(rng, (S, L)) & np.uint32(0xFFFFFFFE)
        for s in range(S):
            d = 37 * s
            for lo, hi in ((0, 3), (40 + d, 90 + d), (TILE, 3 * TILE), (4 * TILE - 100 + d, 4 * TILE + 100 + d),
                           (6 * TILE - 1, 6 * TILE + 1), (63 * TILE + d, 65 * TILE + 5 + d),
                           (L - min(70 + d, L // 3), L)):
                k[s, max(lo, 0):max(min(hi, L), 0)] = SENTINEL
    elif family == 'edges':
        k = EDGE_KEYS[rng.integers(0, len(EDGE_KEYS), (S, L))]
    elif family == 'skew':
        # all but 7 elements share one key (one digit in every pass): the carried row of seg_rowscan_kernel runs up to L
        base = _u32(rng, (S, 1))
        k = np.repeat(base, L, 1)
        for s in range(S):
            at = rng.choice(L, 7, replace=False)
            k[s, at] = base[s, 0] ^ (np.uint32(0x01010101) * (1 + rng.choice(255, 7, replace=False)).astype(np.uint32))
    else:
        raise KeyError(family)
    k = np.ascontiguousarray(k, np.uint32)
    k.setflags(write=False)
    return k


@functools.lru_cache(maxsize=None)
def make_vals(kind, S, L):
    rng = np.random.default_rng([7, S, L])
    if kind == 'arbitrary':
        v = _u32(rng, (S, L))
    else:   # what the losses pass: the element's index in its segment, bit 31 = foreground on a random 40 %
        v = np.arange(L, dtype=np.uint32)[None] | ((rng.random((S, L)) < 0.4).astype(np.uint32) << np.uint32(31))
    v = np.ascontiguousarray(v, np.uint32)
    v.setflags(write=False)
    return v


def expected(keys, vals):
    perm = np.argsort(keys, axis=1, kind='stable')
    return np.take_along_axis(keys, perm, 1), np.take_along_axis(vals, perm, 1)


def _dev(a, dev):
    return torch.from_numpy(np.array(a).view(np.int32).reshape(-1)).to(dev)


def _guarded(n, dev):
    return torch.full((n + 2 * GUARD,), GUARD_WORD, dtype=torch.int32, device=dev)


def device_sort(dev, keys, vals, ws=None):
    """(sorted keys, sorted values, workspace) with the guard words on both sides of both outputs checked"""
    from ssseg import native as N
    S, L = keys.shape
    kin, vin = _dev(keys, dev), _dev(vals, dev)
    kout, vout = _guarded(S * L, dev), _guarded(S * L, dev)
    nb = N.lib().ssseg_lovasz_sort_workspace_bytes(S, L)
    assert nb >= 8 * S * L + 4 * S * 256 * (tiles(L) + 4)
    if ws is None:
        ws = N.workspace(nb, dev)
        ws.fill_(0xC3)
    N.call('ssseg_lovasz_sort', N.dev_ptr(kin), N.dev_ptr(vin), kout.data_ptr() + 4 * GUARD,
           vout.data_ptr() + 4 * GUARD, S, L, N.dev_ptr(ws), nb, N.stream())
    torch.cuda.synchronize()
    assert np.array_equal(kin.cpu().numpy().view(np.uint32), keys.reshape(-1)), 'the input keys were modified'
    assert np.array_equal(vin.cpu().numpy().view(np.uint32), vals.reshape(-1)), 'the input values were modified'
    out = []
    for t in (kout, vout):
        a = t.cpu().numpy().view(np.uint32)
        assert np.all(a[:GUARD] == GUARD_WORD) and np.all(a[GUARD + S * L:] == GUARD_WORD), 'guard words overwritten'
        out.append(a[GUARD:GUARD + S * L].reshape(S, L))
    return out[0], out[1], ws


def check(dev, keys, vals):
    want_k, want_v = expected(keys, vals)
    k1, v1, ws = device_sort(dev, keys, vals)
    bad = np.flatnonzero((k1 != want_k).reshape(-1) | (v1 != want_v).reshape(-1))
    assert bad.size == 0, f'{bad.size} of {k1.size} outputs differ, the first at segment {bad[0] // keys.shape[1]} ' \
                          f'position {bad[0] % keys.shape[1]}'
    assert np.array_equal(k1, want_k) and np.array_equal(v1, want_v)
    k2, v2, _ = device_sort(dev, keys, vals, ws)    # the workspace now holds the first run's tables
    assert np.array_equal(k2, k1) and np.array_equal(v2, v1)
    return k1, v1


@pytest.mark.parametrize('family', FAMILIES)
@pytest.mark.parametrize('L', LENGTHS)
def test_sort_lengths(hip_device, L, family):
    """two segments of every length on the wave, tile and scan-round edges, every key family"""
    assert [tiles(v) for v in (131072, 131073, 262145)] == [SCAN_ROUND, SCAN_ROUND + 1, 2 * SCAN_ROUND + 1]
    keys, vals = make_keys(family, 2, L), make_vals('index', 2, L)
    k, v = check(hip_device, keys, vals)
    if family == 'equal':       # pure stability: the values come out as they went in
        assert np.array_equal(v, vals)
    if family == 'sentinel':    # the ignored pixels' key ends up last, in index order
        for s in range(2):
            n = int((keys[s] == SENTINEL).sum())
            assert n > 0 and np.all(k[s, L - n:] == SENTINEL) and np.all(k[s, :L - n] != SENTINEL)
            assert np.array_equal(v[s, L - n:] & 0x7FFFFFFF, np.flatnonzero(keys[s] == SENTINEL))


@pytest.mark.parametrize('family', ['uniform', 'equal', 'byte0', 'byte3', 'alternate', 'edges'])
@pytest.mark.parametrize('S,L', SHAPES)
def test_sort_segment_shapes(hip_device, S, L, family):
    """several segments of several tiles, and the largest number of segments (gridDim.y = 65,535)"""
    assert 1 <= S <= MAX_S and max(s for s, _ in SHAPES) == MAX_S
    check(hip_device, make_keys(family, S, L), make_vals('index', S, L))


def test_sort_heavy_skew(hip_device):
    """all but 7 of 262,145 elements in one digit of every pass: the carried row holds counts above 2^17 in its
    second and third round"""
    S, L = 2, 262145
    keys = make_keys('skew', S, L)
    for s in range(S):
        u, c = np.unique(keys[s], return_counts=True)
        assert c.max() == L - 7 > 1 << 17 and u.size == 8
        major = u[c.argmax()]
        for shift in (0, 8, 16, 24):    # none of the 7 shares a digit with the rest in any pass
            assert np.all(((u[u != major] >> shift) & 255) != ((major >> shift) & 255))
    check(hip_device, keys, make_vals('index', S, L))


@pytest.mark.parametrize('S,L', [(2, 2049), (3, 131073)])
def test_sort_arbitrary_values(hip_device, S, L):
    """the values are carried, never read: any 32-bit pattern"""
    check(hip_device, make_keys('byte1', S, L), make_vals('arbitrary', S, L))


def test_sort_in_place(hip_device):
    """the outputs may be the inputs (the losses sort in place)"""
    from ssseg import native as N
    S, L = 3, 4097
    keys, vals = make_keys('uniform', S, L), make_vals('index', S, L)
    want_k, want_v = expected(keys, vals)
    k, v = _dev(keys, hip_device), _dev(vals, hip_device)
    nb = N.lib().ssseg_lovasz_sort_workspace_bytes(S, L)
    ws = N.workspace(nb, hip_device)
    N.call('ssseg_lovasz_sort', N.dev_ptr(k), N.dev_ptr(v), N.dev_ptr(k), N.dev_ptr(v), S, L, N.dev_ptr(ws), nb,
           N.stream())
    torch.cuda.synchronize()
    assert np.array_equal(k.cpu().numpy().view(np.uint32).reshape(S, L), want_k)
    assert np.array_equal(v.cpu().numpy().view(np.uint32).reshape(S, L), want_v)


def test_sort_rejects_out_of_bounds_and_short_workspace(hip_device):
    """outside 1 <= S <= 65,535, 1 <= L <= 2^24: SSSEG_EINVAL before anything is launched (the outputs keep their
    fill); a workspace one byte short, or none: SSSEG_EWORKSPACE"""
    from ssseg import native as N
    lib = N.lib()
    buf = [torch.full((64,), 7, dtype=torch.int32, device=hip_device) for _ in range(4)]
    ws = N.workspace(1 << 20, hip_device)
    ptr = [N.dev_ptr(b) for b in buf]
    for S, L in ((MAX_S + 1, 3), (1, MAX_L + 1), (0, 3), (3, 0), (-1, 3), (3, -1)):
        assert lib.ssseg_lovasz_sort_workspace_bytes(S, L) == 0
        assert lib.ssseg_lovasz_sort(*ptr, S, L, N.dev_ptr(ws), 1 << 20, N.stream()) == -1
    assert lib.ssseg_lovasz_sort_workspace_bytes(MAX_S, 3) > 0 and lib.ssseg_lovasz_sort_workspace_bytes(1, MAX_L) > 0
    for i in range(4):
        args = list(ptr)
        args[i] = None
        assert lib.ssseg_lovasz_sort(*args, 2, 8, N.dev_ptr(ws), 1 << 20, N.stream()) == -1
    nb = lib.ssseg_lovasz_sort_workspace_bytes(2, 8)
    assert 0 < nb <= 1 << 20
    assert lib.ssseg_lovasz_sort(*ptr, 2, 8, N.dev_ptr(ws), nb - 1, N.stream()) == -3
    assert lib.ssseg_lovasz_sort(*ptr, 2, 8, None, nb, N.stream()) == -3
    torch.cuda.synchronize()
    assert all(bool((b == 7).all()) for b in buf)
    assert lib.ssseg_lovasz_sort(*ptr, 2, 8, N.dev_ptr(ws), nb, N.stream()) == 0
    torch.cuda.synchronize()
