"""CPU-only checks of tests/philox_ref.py, the host restatement the device draws are pinned to
(tests/test_device_rng.py): the published Philox4x32-10 known-answer vectors, the Box-Muller edges, the counter
bookkeeping of the consumers, and that each comparator of the GPU file rejects a reference with nine rounds, with sin and
cos exchanged, with another stream word and with the carry into c1 dropped."""
import numpy as np
import pytest

import philox_ref as P

OFFSETS = tuple(dict.fromkeys(P.HOST_OFFSETS + P.DEV_COUNTERS))


def _words(hexes):
    return [int(h, 16) for h in hexes.split()]


@pytest.mark.parametrize('ctr,key,out', [
    ('00000000 00000000 00000000 00000000', '00000000 00000000', '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ('ffffffff ffffffff ffffffff ffffffff', 'ffffffff ffffffff', '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ('243f6a88 85a308d3 13198a2e 03707344', 'a4093822 299f31d0', 'd16cfe09 94fdcceb 5001e420 24126ea1'),
])
def test_known_answers(ctr, key, out):
    c, k = _words(ctr), _words(key)
    got = P.philox(c[0] | c[1] << 32, c[2], c[3], k[0] | k[1] << 32)
    assert got.dtype == np.uint32 and got.shape == (1, 4)
    assert got[0].tolist() == _words(out)
    # vectorised over the counters: the same block among others, and the mutations change it
    many = P.philox(np.array([5, c[0] | c[1] << 32, 7], dtype=np.uint64), c[2], c[3], k[0] | k[1] << 32)
    assert many[1].tolist() == _words(out) and many[0].tolist() != many[2].tolist()
    assert P.philox(c[0] | c[1] << 32, c[2], c[3], k[0] | k[1] << 32, rounds=9)[0].tolist() != _words(out)


def test_counters_wrap():
    assert P.counters(2 ** 64 - 2, 4).tolist() == [2 ** 64 - 2, 2 ** 64 - 1, 0, 1]
    assert P.counters(2 ** 32 - 3, 5).tolist() == [2 ** 32 - 3, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1]
    w = P.philox(P.counters(2 ** 32 - 1, 2), 0, 0, 1)
    assert w[1].tolist() == P.philox(2 ** 32, 0, 0, 1)[0].tolist() != P.philox(0, 0, 0, 1)[0].tolist()
    assert P.philox(2 ** 32, 0, 0, 1, carry=False)[0].tolist() == P.philox(0, 0, 0, 1)[0].tolist()


def test_box_muller_edges():
    top, zero = np.uint32((2 ** 24 - 1) << 8), np.uint32(0)
    # c >> 8 = 2^24 - 1: k + 0.5f rounds to 2^24, u1 == 1, both normals exactly 0 whatever the angle
    z, rad = P.box_muller(np.array([[top, np.uint32(0x12345678), top, top]], dtype=np.uint32), 6.283185307179586)
    assert (z == 0).all() and (rad == 0).all()
    # the smallest u1 = 2^-25: the largest radius, sqrt(2 ln 2^25) = 5.887...; u2 = 0: cos = 1, sin = 0
    z, rad = P.box_muller(np.array([[zero, zero, zero, top]], dtype=np.uint32), 6.283185307179586)
    assert abs(rad[0, 0] - np.sqrt(2 * 25 * np.log(2.0))) < 1e-12 and 5.887 < rad[0, 0] < 5.89
    assert z[0, 0] == rad[0, 0] and z[0, 1] == 0 and abs(z[0, 2]) <= rad[0, 0] and abs(z[0, 3]) < 1e-5
    # pairs do not share a uniform: z[0], z[1] come from (c0, c1) alone, z[2], z[3] from (c2, c3) alone
    a = np.array([[1 << 20, 2 << 20, 3 << 20, 4 << 20]], dtype=np.uint32)
    b = np.array([[1 << 20, 2 << 20, 5 << 20, 6 << 20]], dtype=np.uint32)
    za, zb = P.box_muller(a, 6.283185307179586)[0], P.box_muller(b, 6.283185307179586)[0]
    assert (za[0, :2] == zb[0, :2]).all() and (za[0, 2:] != zb[0, 2:]).all()
    for seed in P.SEEDS:
        z, rad = P.normals(4 * 4096 + 3, seed, 2 ** 32 - 3, with_rad=True)
        assert z.shape == (4 * 4096 + 3,) and float(np.abs(z).max()) <= 5.89 and (np.abs(z) <= rad).all()
        assert abs(float(z.mean())) < 0.04 and abs(float(z.std()) - 1) < 0.03      # 5 sigma at n = 16387


def _trace(monkeypatch):
    """record (word2, word3, counters) of every philox call"""
    calls, real = [], P.philox

    def spy(ctr, word2, word3, seed, **kw):
        c = np.atleast_1d(np.asarray(ctr, dtype=np.uint64))
        calls.append((np.broadcast_to(np.asarray(word2, dtype=np.uint64), c.shape).copy(), int(word3), c.copy()))
        return real(ctr, word2, word3, seed, **kw)
    monkeypatch.setattr(P, 'philox', spy)
    return calls


def test_consecutive_calls_use_disjoint_counters(monkeypatch):
    """A step's consumers called one after the other, each at the counter the documented advances leave: no
    (stream word, counter) pair is drawn twice, every call stays within [start, start + advance), and the stream words
    of the consumers that share the counter are pairwise distinct."""
    words = (P.STREAM_NOISE, P.STREAM_PSIGMA, P.STREAM_AFFINE, P.STREAM_KEYS, P.STREAM_PARAMS)
    assert len(set(words)) == len(words) == 5
    for start in P.DEV_COUNTERS:
        calls = _trace(monkeypatch)
        ctr, spans = start, []
        for _ in range(2):
            for B, HW, C in ((1, 1, 1), (3, 5, 5), (4, 64, 19), (65, 7, 64)):
                a = P.cowmix_draw(B, HW, (0.3, 0.7, 1, 6), 7, ctr)['advance']
                assert a == B + -(-B * HW // 4) + 1
                spans.append((len(calls), ctr, a))
                ctr += a
                P.affine_draw(B, 24, 32, 15, 0.75, 1.25, 7, ctr)
                spans.append((len(calls), ctr, B))
                ctr += B
                a = P.mixmask_draw(B, C, 7, ctr)[2]
                assert a == B * (-(-C // 4) + 1)
                spans.append((len(calls), ctr, a))
                ctr += a
        seen, first = set(), 0
        for upto, begin, adv in spans:
            for w2, w3, c in calls[first:upto]:
                rel = (c - np.uint64(begin % 2 ** 64)).astype(np.uint64)        # mod 2^64
                assert w3 == 0 and int(rel.max()) < adv, (begin, adv, int(rel.max()))
                pairs = set(zip(w2.tolist(), c.tolist()))
                assert len(pairs) == c.size and not (pairs & seen)
                seen |= pairs
            first = upto
        assert {w for w, _ in seen} == set(words)
        monkeypatch.undo()
    # dropout: ssseg_rng_take reserves ceil(n/4) + 1 per call, the kernel draws n/4 counters of a stream of its own
    calls = _trace(monkeypatch)
    P.dropout_mask(1028, 0.5, 7, 2 ** 32 - 3)
    P.dropout_mask(1028, 0.5, 7, 2 ** 32 - 3 + 1028 // 4 + 1)
    (wa, _, ca), (wb, _, cb) = calls
    assert set(wa.tolist()) == set(wb.tolist()) == {P.STREAM_DROPOUT} and not set(ca.tolist()) & set(cb.tolist())
    assert P.STREAM_DROPOUT not in words and P.STREAM_FIELD not in words + (P.STREAM_DROPOUT,)


# ---- the comparators can fail ----------------------------------------------------------------------------------------
MUTATIONS = {'nine rounds': dict(rounds=9), 'carry dropped': dict(carry=False)}


def _rejects(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


def _carry_live(offset, ncounters):
    """whether some counter of the call has c1 != 0"""
    return bool((P.counters(offset, ncounters) >> np.uint64(32)).any())


def _mutants(case, offset, ncounters, extra):
    """(name, kwargs) of the mutations that can show at this offset"""
    out = list(extra.items()) + [('nine rounds', MUTATIONS['nine rounds'])]
    if _carry_live(offset, ncounters):
        out.append(('carry dropped', MUTATIONS['carry dropped']))
    return out


def test_comparators_accept_the_reference_and_reject_mutants():
    """At the smallest shape of each GPU test and every (seed, counter) of the suite: the comparator accepts the
    reference rounded to the device's type and rejects the reference built with nine rounds, with sin and cos
    exchanged (where the consumer has them), with another consumer's stream word, and with c1 forced to 0 (wherever
    some counter of the call has c1 != 0: at 2^64 - 2 and 2^33 - 1 for a one-counter call, at 2^32 - 3 too once the call
    draws more than three)."""
    tally = {}

    def note(cmp, name, rejected):
        tally.setdefault((cmp, name), []).append(rejected)

    H, W = P.AFFINE_HW
    for seed in P.SEEDS:
        for off in OFFSETS:
            # normals, n = 1: one counter
            n = P.NORMAL_SIZES[0]
            got = P.normals(n, seed, off).astype(np.float32)
            assert P.check_normals(got, *P.normals(n, seed, off, True)) <= 1.0
            for name, mut in _mutants('normals', off, 1, {'sin / cos': dict(swap=True), 'stream 1': dict(word2=1)}):
                note('normals', name, _rejects(P.check_normals, got, *P.normals(n, seed, off, True, **mut)))
            # ClassMix keys and CutMix params, (B, C) = (1, 4): counters off (keys) and off + 1 (params)
            B, C = P.MIXMASK_SHAPES[0]
            keys, params, _ = P.mixmask_draw(B, C, seed, off)
            for name, mut in _mutants('mixmask', off, 2, {'stream 1': dict(word2=1, params_word2=1),
                                                           'streams exchanged': dict(word2=4, params_word2=3)}):
                k, p, _ = P.mixmask_draw(B, C, seed, off, **mut)
                if name != 'carry dropped' or _carry_live(off, 1):
                    note('keys', name, _rejects(P.check_exact, keys, k))
                note('params', name, _rejects(P.check_exact, params, p))
            # dropout, n = 4: four mask bits, which a mutant matches by chance once in 16
            n = P.DROPOUT_SIZES[0]
            m = P.dropout_mask(n, 0.5, seed, off)
            for name, mut in _mutants('dropout', off, 1, {'stream 1': dict(word2=1)}):
                note('dropout', name, _rejects(P.check_exact, m, P.dropout_mask(n, 0.5, seed, off, **mut)))
            # CowMix p (exact and general) and sigma, B = 1: one counter; the noise: two more
            rng = P.END_TO_END[2][1]
            d = P.cowmix_draw(1, P.COWMIX_HW, (0, 1) + rng[2:], seed, off)
            g = P.cowmix_draw(1, P.COWMIX_HW, rng, seed, off)
            p32, s32, z32 = g['p'].astype(np.float32), g['sigma'].astype(np.float32), g['noise'].astype(np.float32)
            assert P.check_ulp(p32, g['p']) <= 1.0 and P.check_sigma(s32, g['sigma'], g['a'], *rng[2:]) <= 1.0
            for name, mut in _mutants('cowmix', off, 1, {'stream 0': dict(word2=0)}):
                dm, gm = P.cowmix_draw(1, P.COWMIX_HW, (0, 1) + rng[2:], seed, off, **mut), \
                    P.cowmix_draw(1, P.COWMIX_HW, rng, seed, off, **mut)
                note('p exact', name, _rejects(P.check_exact, d['p_unit'], gm['p_unit']))
                note('p ulp', name, _rejects(P.check_ulp, p32, gm['p']))
                note('sigma', name, _rejects(P.check_sigma, s32, gm['sigma'], gm['a'], *rng[2:]))
                assert dm['p_unit'].tolist() == gm['p_unit'].tolist() == dm['p'].tolist()
            for name, mut in _mutants('cowmix noise', off + 1, 2, {'sin / cos': dict(swap=True),
                                                                  'stream 1': dict(noise_word2=1)}):
                gm = P.cowmix_draw(1, P.COWMIX_HW, rng, seed, off, **mut)
                note('cowmix noise', name, _rejects(P.check_normals, z32, gm['noise'], gm['rad']))
            # affine, B = 1
            _, _, a, ai = P.affine_draw(1, H, W, *P.AFFINE_RANGE, seed, off)
            a32, ai32 = a.astype(np.float32), ai.astype(np.float32)
            assert P.check_affine(a32, a, H, W) <= 1.0 and P.check_affine(ai32, ai, H, W) <= 1.0
            for name, mut in _mutants('affine', off, 1, {'stream 1': dict(word2=1)}):
                _, _, b, bi = P.affine_draw(1, H, W, *P.AFFINE_RANGE, seed, off, **mut)
                note('affine', name, _rejects(P.check_affine, a32, b, H, W))
                note('affine inverse', name, _rejects(P.check_affine, ai32, bi, H, W))
        # the uniform field, n = 1 (its counter starts at 0 in every call: no carry to drop)
        f = P.uniform_field(P.FIELD_SIZES[0], seed)
        for name, mut in (('nine rounds', dict(rounds=9)), ('stream 0x5eed', dict(word2=P.STREAM_DROPOUT))):
            note('field', name, _rejects(P.check_exact, f, P.uniform_field(P.FIELD_SIZES[0], seed, **mut)))
    for (cmp, name), r in sorted(tally.items()):
        print(f'{cmp:15s} {name:18s} rejected in {sum(r)} of {len(r)} cases')
        if cmp == 'dropout':
            assert len(r) >= 6 and sum(r) >= len(r) // 2, (cmp, name, r)      # 4 bits: 15 of 16 expected
        else:
            assert len(r) >= 3 and all(r), (cmp, name, r)
    names = {c: {n for cc, n in tally if cc == c} for c, _ in tally}
    for c in ('normals', 'keys', 'params', 'dropout', 'p exact', 'p ulp', 'sigma', 'cowmix noise', 'affine',
              'affine inverse'):
        assert {'nine rounds', 'carry dropped'} <= names[c] and any(n.startswith('stream') for n in names[c]), c
    assert 'sin / cos' in names['normals'] and 'sin / cos' in names['cowmix noise']


def test_mask_comparator_rejects_mutants():
    """the end-to-end comparator at its smallest shape, (2, 61, 67), counter 2^32 - 3 (the noise starts at 2^32 - 1)"""
    (B, H, W), rng = P.END_TO_END[2]
    seed, off = P.SEEDS[1], 2 ** 32 - 3
    ref = P.cowmix_reference(B, H, W, rng, seed, off)
    frac, inside, r = P.check_masks(ref['mask'], ref['thr'], ref)
    print(f'band holds {frac:.5f} of the pixels; K clearance {ref["k_clearance"]:.4f}')
    assert inside == 0 and r == 0.0 and 0.3 < float(ref['mask'].mean()) < 0.7
    for name, mut in (('nine rounds', dict(rounds=9)), ('sin / cos', dict(swap=True)), ('carry dropped', dict(carry=False)),
                      ('noise on stream 1', dict(noise_word2=1)), ('p / sigma on stream 0', dict(word2=0))):
        assert _rejects(P.check_masks, ref['mask'], ref['thr'], P.cowmix_reference(B, H, W, rng, seed, off, **mut)), name
    # one pixel outside the band, and a threshold off by more than its bound
    far = np.unravel_index(np.argmax(np.abs(ref['field'] - ref['thr'][:, None, None])), ref['field'].shape)
    flipped = ref['mask'].copy()
    flipped[far] = 1 - flipped[far]
    assert _rejects(P.check_masks, flipped, ref['thr'], ref)
    assert _rejects(P.check_masks, ref['mask'], ref['thr'] + np.float32(1e-4), ref)


def test_level_comparator_rejects_mutants():
    """the ISO hue comparator at the GPU test's shape: n = 3, 64 x 64, sample 1 with colour std 20"""
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, size=(3, 64, 64, 3)).astype(np.float32)
    std = (0.0, 20.0, None)
    ref = P.iso_reference(img, std, 1234)
    P.check_levels(ref.astype(np.float32), ref)
    for name, mut in (('nine rounds', dict(rounds=9)), ('sin for cos', dict(swap=True)), ('c3 = 0', dict(word3=0))):
        assert _rejects(P.check_levels, ref.astype(np.float32), P.iso_reference(img, std, 1234, **mut)), name
    # the image index is the stream word c2: another image's noise is rejected too
    other = P.iso_reference(img[[0, 2, 1]], (0.0, None, 20.0), 1234)[[0, 2, 1]]
    assert _rejects(P.check_levels, ref.astype(np.float32), other)
    # without noise (the conversion chain alone) the hue test would not pass either: it does test the noise
    assert _rejects(P.check_levels, ref.astype(np.float32), P.iso_reference(img, (0.0, 0.0, None), 1234))
