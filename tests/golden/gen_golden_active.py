"""Writes tests/golden/active_entropy.npz: small logit maps and the fp64 value of the reference's entropy expression
on each of them (get_active_learning_partition.py:94-95: probs = softmax(logits, dim=1); entropy =
-(probs * log(probs)).sum(dim=1).mean(), one image at a time).  The reference script cannot be imported (it opens a
database connection at import), so the stated expression is evaluated here with torch in fp64.  Only inputs on which
that expression is finite are stored: it is NaN once a probability underflows, which is where the device kernel
deviates on purpose.

    python tests/golden/gen_golden_active.py
"""
import os

import numpy as np
import torch

SHAPES = [(1, 2, 1, 1), (3, 2, 1, 3), (2, 3, 5, 7), (2, 19, 9, 11), (1, 64, 4, 5)]


def main():
    out = {}
    for n, shape in enumerate(SHAPES):
        g = torch.Generator().manual_seed(700 + n)
        x = (torch.randn(*shape, generator=g) * 3).float()
        ent = []
        for b in range(shape[0]):
            probs = torch.softmax(x[b:b + 1].double(), dim=1)
            ent.append(float(-(probs * torch.log(probs)).sum(dim=1).mean()))
        assert np.isfinite(ent).all(), shape
        out[f'logits{n}'] = x.numpy()
        out[f'entropy{n}'] = np.asarray(ent, np.float64)
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'active_entropy.npz'), **out)


if __name__ == '__main__':
    main()
