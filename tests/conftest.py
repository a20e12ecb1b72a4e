import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'semi-supervised_semantic_segmentation_amd')
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)


def pytest_configure(config):
    config.addinivalue_line('markers', 'gpu: needs a real MI355X (HIP device)')


class _GoldenParts:
    """A fixture that gen_golden.py cut into name.npz, name.part1.npz, ... (no committed file over 1 MiB), read as one
    NpzFile-like mapping: the same keys in the same order."""

    def __init__(self, parts):
        self._where = {k: p for p in parts for k in p.files}
        self.files = list(self._where)

    def __getitem__(self, key):
        return self._where[key][key]

    def __contains__(self, key):
        return key in self._where

    def __iter__(self):
        return iter(self.files)

    def __len__(self):
        return len(self.files)

    def keys(self):
        return self._where.keys()


def golden(name):
    first = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
    parts, n = [first], 1
    while os.path.exists(os.path.join(GOLDEN, f'{name[:-4]}.part{n}.npz')):
        parts.append(np.load(os.path.join(GOLDEN, f'{name[:-4]}.part{n}.npz'), allow_pickle=False))
        n += 1
    return first if n == 1 else _GoldenParts(parts)


@pytest.fixture(scope='session')
def hip_device():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no HIP device')
    return torch.device('cuda:0')
