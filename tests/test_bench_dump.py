"""bench.py --dump-outputs (bench.dump_outputs) on the host: the files it writes, their dtype and order, and the fixed
seeded sample a model larger than bench.DUMP_SAMPLE is cut to."""
import os

import numpy as np
import torch


def _models():
    torch.manual_seed(5)
    student = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4))
    teacher = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.BatchNorm2d(4))
    rec = (torch.tensor(0.25), torch.tensor(1.5, dtype=torch.bfloat16), torch.tensor(0.5))
    return student, teacher, rec


def _flat(m):
    return torch.cat([v.float().reshape(-1) for v in m.state_dict().values() if v.is_floating_point()]).numpy()


def test_dump_outputs_whole_state(tmp_path):
    import bench
    student, teacher, rec = _models()
    out = str(tmp_path / 'dump')
    bench.dump_outputs(out, student, teacher, rec)
    assert sorted(os.listdir(out)) == ['losses.npy', 'student_state.npy', 'teacher_state.npy']
    losses = np.load(os.path.join(out, 'losses.npy'))
    assert losses.dtype == np.float32 and losses.tolist() == [0.25, 1.5, 0.5]
    for name, m in (('student_state', student), ('teacher_state', teacher)):
        a = np.load(os.path.join(out, name + '.npy'))
        # weights, bias, BN affine and running statistics; the integer num_batches_tracked is left out
        assert a.dtype == np.float32 and a.shape == (3 * 4 * 9 + 4 + 4 * 4,)
        assert np.array_equal(a, _flat(m))


def test_dump_outputs_sample_is_fixed(tmp_path, monkeypatch):
    import bench
    student, teacher, rec = _models()
    monkeypatch.setattr(bench, 'DUMP_SAMPLE', 32)
    a_dir, b_dir = str(tmp_path / 'a'), str(tmp_path / 'b')
    bench.dump_outputs(a_dir, student, teacher, rec)
    with torch.no_grad():
        student[0].weight.add_(1.0)
    bench.dump_outputs(b_dir, student, teacher, rec)
    g = torch.Generator().manual_seed(bench.DUMP_SAMPLE_SEED)
    idx = torch.randint(128, (32,), generator=g).sort().values.numpy()
    a, b = (np.load(os.path.join(d, 'student_state.npy')) for d in (a_dir, b_dir))
    assert a.shape == b.shape == (32,)
    assert np.array_equal(b, _flat(student)[idx])        # the same positions on every call
    assert np.array_equal((b - a) != 0, idx < 108)       # only the sampled conv weights moved
    assert np.array_equal(np.load(os.path.join(a_dir, 'teacher_state.npy')),
                          np.load(os.path.join(b_dir, 'teacher_state.npy')))
