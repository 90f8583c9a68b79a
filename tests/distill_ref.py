"""float64 torch restatement of the flow distillation term (csrc/pwc_distill.hip, pwcnet_amd.unsup.flow_distill_*): the reference
of tests/test_gpu_distill.py, itself checked against hand values and its closed-form gradient by tests/test_host_distill.py.

    student (N, h, w, 2), teacher (N, H, W, 2), offset (y0, x0): student pixel p = (y, x) pairs with teacher pixel P = (y + y0, x + x0)
    p contributes iff teacher_valid[P] (where given), not exclude[p] (where given), both teacher components at P finite with
    |.| <= 1e9, both student components at p finite
    sums[n] = sum over the contributing p of rho(student[p,0] - teacher[P,0]) + rho(student[p,1] - teacher[P,1]),  rho(d) = (d^2 + eps^2)^q
"""
import numpy as np
import torch

SENTINEL = 1e9


def window(t, offset, h, w):
    y0, x0 = offset
    return t[:, y0:y0 + h, x0:x0 + w]


def contributes(student, teacher, offset=(0, 0), teacher_valid=None, exclude=None):
    """(N, h, w) torch.bool."""
    N, h, w, _ = student.shape
    t = window(teacher, offset, h, w)
    c = torch.isfinite(t).all(-1) & (t.abs() <= SENTINEL).all(-1) & torch.isfinite(student).all(-1)
    if teacher_valid is not None:
        c = c & (window(teacher_valid, offset, h, w) != 0)
    if exclude is not None:
        c = c & (exclude == 0)
    return c


def differences(student, teacher, offset, c):
    """student - teacher through the window in float64, 0 where the pixel does not contribute (no NaN leaves here)."""
    N, h, w, _ = student.shape
    t = window(teacher, offset, h, w).detach().double()
    s = student.double()
    m = c.unsqueeze(-1)
    return torch.where(m, s, torch.zeros_like(s)) - torch.where(m, t, torch.zeros_like(t))


def distill_sums(student, teacher, offset=(0, 0), teacher_valid=None, exclude=None, eps=1e-3, q=0.5):
    """(sums (N,) float64, counts (N,) int64); differentiable w.r.t. student."""
    c = contributes(student.detach(), teacher.detach(), offset, teacher_valid, exclude)
    d = differences(student, teacher, offset, c)
    rho = (d * d + float(eps) ** 2) ** float(q)
    rho = torch.where(c.unsqueeze(-1), rho, torch.zeros_like(rho))
    return rho.sum(dim=(1, 2, 3)), c.sum(dim=(1, 2))


def distill_loss(student, teacher, offset=(0, 0), teacher_valid=None, exclude=None, eps=1e-3, q=0.5):
    sums, counts = distill_sums(student, teacher, offset, teacher_valid, exclude, eps, q)
    return sums.sum() / (2.0 * counts.sum().clamp(min=1).double())


def distill_grad(student, teacher, dsums, offset=(0, 0), teacher_valid=None, exclude=None, eps=1e-3, q=0.5):
    """The closed form: dsums[n] * 2 q d (d^2 + eps^2)^(q - 1) at the contributing pixels, 0 elsewhere; (N, h, w, 2) float64."""
    c = contributes(student, teacher, offset, teacher_valid, exclude)
    d = differences(student, teacher, offset, c)
    g = dsums.double().reshape(-1, 1, 1, 1) * 2.0 * float(q) * d * (d * d + float(eps) ** 2) ** (float(q) - 1.0)
    return torch.where(c.unsqueeze(-1), g, torch.zeros_like(g))


def random_case(N, h, w, H, W, seed, spread=2.0):
    """Seeded float32 flows and masks for the mask tests: student (N,h,w,2), teacher (N,H,W,2), teacher_valid (N,H,W) and exclude
    (N,h,w) uint8.  Three in ten of the teacher's pixels hold the .flo sentinel 1e10 in one component, teacher_valid keeps about 60 %
    and exclude drops about 40 %: with no mask about 70 % of the pixels contribute, with either mask 42 %, with both 25 % -- the
    tests assert 10 % .. 90 % per image in the restatement, so that a mask bug cannot hide behind an empty or a full set."""
    rng = np.random.RandomState(seed)
    student = rng.normal(0.0, spread, size=(N, h, w, 2)).astype(np.float32)
    teacher = rng.normal(0.0, spread, size=(N, H, W, 2)).astype(np.float32)
    unknown = rng.uniform(size=(N, H, W)) < 0.3
    teacher[..., 0][unknown & (rng.uniform(size=(N, H, W)) < 0.5)] = 1e10
    teacher[..., 1][unknown & (teacher[..., 0] != 1e10)] = 1e10
    teacher_valid = (rng.uniform(size=(N, H, W)) < 0.6).astype(np.uint8)
    exclude = (rng.uniform(size=(N, h, w)) < 0.4).astype(np.uint8)
    return tuple(torch.from_numpy(a) for a in (student, teacher, teacher_valid, exclude))
