"""The synthetic arena of the fused parameter-step tests (test_param_step.py on the device, test_param_step_host.py
for the descriptor grouping): four conv weights with 1, 2, 4 and 10 packs and ranges of 1, 255 and 1027 elements
without packs between them, laid out like ssseg.arena.FlatArena does (every slot starts at a multiple of 4 elements).

A pack spec is the ssseg_weight_pack argument tuple (Kd, Kr, Cd, Rs, Ss, Cp, layout, r0, rstep, Rn, s0, sstep, Sn).
"""


def _full(Kd, Kr, Cd, R, S, Cp, layout, flip=False):
    if flip:
        return (Kd, Kr, Cd, R, S, Cp, layout, R - 1, -1, R, S - 1, -1, S)
    return (Kd, Kr, Cd, R, S, Cp, layout, 0, 1, R, 0, 1, S)


def _phases(Kd, Kr, Cd, Cp):
    """the four stride-2 output phases of a 4x4 ConvTranspose2d forward (layout 1)"""
    return [(Kd, Kr, Cd, 4, 4, Cp, 1, r0, 2, 2, s0, 2, 2) for r0 in (0, 1) for s0 in (0, 1)]


# (name, weight shape or range length, [(teacher, spec)])
SLOTS = [
    ('w1', (8, 8, 1, 1), [(0, _full(8, 8, 8, 1, 1, 8, 0))]),
    ('r1', 1, None),
    ('w2', (64, 8, 7, 7), [(0, _full(64, 64, 8, 7, 7, 8, 0)), (0, _full(8, 8, 64, 7, 7, 64, 1, flip=True))]),
    ('r255', 255, None),
    ('w3', (72, 40, 3, 3), [(0, _full(72, 72, 40, 3, 3, 40, 0)), (0, _full(80, 72, 40, 3, 3, 48, 0)),   # padded rows, channels
                            (0, _full(40, 40, 72, 3, 3, 72, 1, flip=True)), (1, _full(72, 72, 40, 3, 3, 40, 0))]),
    ('r1027', 1027, None),
    # ConvTranspose2d weight [Cin 24][Cout 16][4][4]: the forward's four phase packs for student and teacher, the
    # conv over its output gradient (layout 0), and a teacher pack whose channel count is no multiple of 8
    ('wT', (24, 16, 4, 4), [(0, s) for s in _phases(16, 16, 24, 24)] + [(1, s) for s in _phases(16, 16, 24, 24)]
     + [(0, _full(24, 24, 16, 4, 4, 16, 0)), (1, _full(24, 24, 16, 4, 4, 20, 0))]),
    ('r5', 5, None),
]


def layout():
    """[(name, offset, numel, shape or None, packs or None)], arena length"""
    out, pos = [], 0
    for name, what, packs in SLOTS:
        n = what if isinstance(what, int) else what[0] * what[1] * what[2] * what[3]
        out.append((name, pos, n, None if isinstance(what, int) else what, packs))
        pos += (n + 3) // 4 * 4
    return out, pos


def pack_numel(spec):
    Kd, _, _, _, _, Cp, _, _, _, Rn, _, _, Sn = spec
    return Kd * Rn * Sn * Cp
