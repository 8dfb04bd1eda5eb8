"""GPU tests of ``kw_kd_loss`` (csrc/kd.hip) and ``kwhisper.distill.kd_loss``: the temperature KL of kotoba-whisper's
``train_step`` (run_distillation.py:614-622, 652-657), forward and student gradient, against the float64 restatement
tests/_distill_ref.py (which tests/test_distill_cpu.py holds to torch's KLDivLoss expression).

Bars, from f32 arithmetic on |logit / T| <= 100 (unit roundoff 6e-8 x 100 = 6e-6 absolute in an exponent):
  row_kl, loss:  |got - ref| <= 1e-5 + 1e-4 ref
  gradient:      |got - ref| <= 2e-5 T / n_valid   (+ 2^-8 |ref| for a bf16 gradient's final rounding)
Ignored rows are exactly zero in row_kl and in every gradient element; two runs are bitwise equal."""
import numpy as np
import pytest
import torch

import _distill_ref as DR
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs the MI355X")]

F32, BF16 = torch.float32, torch.bfloat16
# (N, V, student dtype, row stride, element offset of the first row in its allocation)
SHAPES = [
    (1, 7, F32, 7, 0),
    (3, 51865, F32, 51865, 0),        # odd V: rows at 4-byte alignment
    (5, 51866, BF16, 51866, 1),       # bf16 rows at 2-byte alignment (odd element offsets 1, 51867, ...)
    (70, 1000, F32, 1024, 0),         # ld > V, more rows than one wave of workgroups per XCD
    (70, 1000, BF16, 1024, 0),
]
IDS = ["1x7-f32", "3x51865-f32", "5x51866-bf16", "70x1000-f32-ld1024", "70x1000-bf16-ld1024"]
TEMPS = [0.5, 1.0, 2.0]
KINDS = ["one_ignored", "extreme", "first_last_ignored", "equal", "all_ignored"]


def _padded(x, ld, off, dtype, fill):
    """x [N][V] on the device as rows of stride ld starting ``off`` elements into an allocation whose every other
    element is ``fill`` (NaN for inputs: a read outside a row poisons the result)."""
    N, V = x.shape
    flat = torch.full((off + N * ld,), fill, device="cuda", dtype=dtype)
    view = flat[off:].view(N, ld)[:, :V]
    view.copy_(torch.from_numpy(x).to("cuda"))
    return flat, view


def _case(kind, N, V, sdt, T, seed):
    rng = np.random.RandomState(seed)
    t = (rng.standard_normal((N, V)) * 3).astype(np.float32)
    s = (rng.standard_normal((N, V)) * 3).astype(np.float32)
    labels = rng.randint(0, V, size=N).astype(np.int64)
    if kind == "extreme":  # entries at +-80 T in both tensors: only the maximum's subtraction keeps exp() finite
        for x in (t, s):
            for r in range(N):
                idx = rng.choice(V, size=min(4, V), replace=False)
                x[r, idx] = (np.array([80, -80, 80, -80][: len(idx)]) * T).astype(np.float32)
    if sdt == BF16:  # the student as the bf16 values the kernel reads
        s = torch.from_numpy(s).to(BF16).float().numpy()
    if kind == "equal":
        t = s.copy()
    if kind in ("one_ignored", "extreme", "equal") and N > 1:
        labels[N // 2] = -100
    if kind == "first_last_ignored":
        labels[0] = labels[-1] = -100
    if kind == "all_ignored":
        labels[:] = -100
    return t, s, labels


def _run(t, s, labels, sdt, ld, off, T):
    from kwhisper import ops

    N, V = t.shape
    _, tv = _padded(t, ld, off, F32, float("nan"))
    _, sv = _padded(s, ld, off, sdt, float("nan"))
    gflat = torch.full((off + N * ld,), 7.0, device="cuda", dtype=sdt)
    gv = gflat[off:].view(N, ld)[:, :V]
    lab = torch.from_numpy(labels).cuda()
    loss, row = ops.kd_loss(tv, sv, lab, T, grad=gv)
    out = (loss.clone(), row.clone(), gflat.clone())
    loss2, row2 = ops.kd_loss(tv, sv, lab, T, grad=gv)  # again, into the same buffers: bitwise the same
    assert torch.equal(loss2.view(torch.int32), out[0].view(torch.int32))
    assert torch.equal(row2.view(torch.int32), out[1].view(torch.int32))
    assert torch.equal(gflat.view(torch.int16 if sdt == BF16 else torch.int32),
                       out[2].view(torch.int16 if sdt == BF16 else torch.int32))
    # nothing outside the rows was written
    pad = torch.ones_like(gflat, dtype=torch.bool)
    pad[off:].view(N, ld)[:, :V] = False
    assert bool((gflat[pad] == 7.0).all())
    # a forward-only call gives the same loss and rows
    loss3, row3 = ops.kd_loss(tv, sv, lab, T)
    assert torch.equal(loss3.view(torch.int32), out[0].view(torch.int32))
    assert torch.equal(row3.view(torch.int32), out[1].view(torch.int32))
    return float(out[0].item()), out[1].double().cpu().numpy(), gv.double().cpu().numpy()


def _check(kind, got, ref, labels, sdt, T):
    loss, row, grad = got
    rloss, rrow, rgrad = ref
    valid = labels >= 0
    n = int(valid.sum())
    assert (row[~valid] == 0).all() and (grad[~valid] == 0).all()
    if n == 0:
        assert np.isnan(loss) and np.isnan(rloss)
        assert (grad == 0).all() and (row == 0).all()
        return
    gbar = 2e-5 * T / n + (2.0 ** -8 * np.abs(rgrad) if sdt == BF16 else 0.0)
    row_err = np.abs(row - rrow)
    print(f"{kind}: loss {loss:.7g} ref {rloss:.7g}; max row err {row_err.max():.3g} (rel "
          f"{(row_err / np.maximum(rrow, 1e-30))[valid].max():.3g}); max grad err {np.abs(grad - rgrad).max():.3g} "
          f"(bar {np.min(gbar):.3g})")
    if kind == "equal":
        assert (row <= 1e-5).all() and (row >= -1e-5).all()
        assert (np.abs(grad) <= gbar).all()
    assert (row_err <= 1e-5 + 1e-4 * rrow).all()
    assert abs(loss - rloss) <= 1e-5 + 1e-4 * rloss
    assert (np.abs(grad - rgrad) <= gbar).all()


@pytest.mark.parametrize("T", TEMPS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_kd_loss_against_f64(shape, kind, T):
    N, V, sdt, ld, off = shape
    t, s, labels = _case(kind, N, V, sdt, T, seed=N + V)
    got = _run(t, s, labels, sdt, ld, off, T)
    _check(kind, got, DR.kd_ref(t, s, labels, T), labels, sdt, T)


def test_kd_loss_ctypes_backend_matches_torch_ops():
    """Both bindings fill the same argument block: bitwise the same results."""
    from kwhisper import ops

    N, V = 4, 333
    t, s, labels = _case("one_ignored", N, V, BF16, 2.0, seed=3)
    tv, sv = torch.from_numpy(t).cuda(), torch.from_numpy(s).cuda().to(BF16)
    lab = torch.from_numpy(labels).cuda()
    res = {}
    old = ops.backend()
    try:
        for b in ("torch", "ctypes"):
            ops.set_backend(b)
            g = torch.empty_like(sv)
            loss, row = ops.kd_loss(tv, sv, lab, 2.0, grad=g)
            res[b] = (loss.clone(), row.clone(), g)
    finally:
        ops.set_backend(old)
    for a, b in zip(res["torch"], res["ctypes"]):
        assert torch.equal(a.view(torch.int16 if a.dtype == BF16 else torch.int32),
                           b.view(torch.int16 if b.dtype == BF16 else torch.int32))


@pytest.mark.parametrize("how", ["step", "slice"])
def test_distill_kd_loss_strided_view_and_autograd(how):
    """[2, 3, 51865] strided views through the public loss: ``step`` keeps one row stride (taken as a view), ``slice``
    does not (copied).  (3 * loss).backward() is 3 x the gradient of the unscaled call; the teacher gets none."""
    from kwhisper.distill import kd_loss

    B, Tn, V, T = 2, 3, 51865, 2.0
    rng = np.random.RandomState(11)
    big = (B, 2 * Tn, V) if how == "step" else (B, Tn + 2, V)
    sel = (slice(None), slice(0, None, 2)) if how == "step" else (slice(None), slice(1, Tn + 1))
    s_base = torch.from_numpy((rng.standard_normal(big) * 3).astype(np.float32)).cuda().requires_grad_(True)
    t_base = torch.from_numpy((rng.standard_normal(big) * 3).astype(np.float32)).cuda().requires_grad_(True)
    labels = torch.from_numpy(rng.randint(0, V, size=(B, Tn))).cuda()
    labels[1, 0] = -100
    loss, row = kd_loss(s_base[sel], t_base[sel], labels, T, return_row_kl=True)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and not row.requires_grad
    loss.backward()
    g1 = s_base.grad.clone()
    assert t_base.grad is None
    s_base.grad = None
    (3 * kd_loss(s_base[sel], t_base[sel], labels, T)).backward()
    g3 = s_base.grad.clone()
    sn = s_base.detach()[sel].reshape(-1, V).cpu().numpy()
    tn = t_base.detach()[sel].reshape(-1, V).cpu().numpy()
    ln = labels.reshape(-1).cpu().numpy()
    rloss, rrow, rgrad = DR.kd_ref(tn, sn, ln, T)
    n = int((ln >= 0).sum())
    assert abs(float(loss.detach()) - rloss) <= 1e-5 + 1e-4 * rloss
    assert (np.abs(row.double().cpu().numpy() - rrow) <= 1e-5 + 1e-4 * rrow).all()
    got = g1[sel].reshape(-1, V).double().cpu().numpy()
    assert (np.abs(got - rgrad) <= 2e-5 * T / n).all()
    assert (got[ln < 0] == 0).all()
    # rows of the base outside the view receive exactly zero
    outside = torch.ones(big[:2], dtype=torch.bool, device="cuda")
    outside[sel] = False
    assert bool((g1[outside] == 0).all())
    # 3 x: a product of f32 values by 3.0, rounded once
    assert torch.equal(g3, g1 * 3)
    # a student that asks for no gradient takes the forward-only launch: the same loss, bit for bit
    with torch.no_grad():
        l0 = kd_loss(s_base[sel], t_base[sel], labels, T)
    assert torch.equal(l0.view(torch.int32), loss.detach().view(torch.int32))


def test_distill_kd_loss_casts_a_bf16_teacher():
    from kwhisper.distill import kd_loss

    rng = np.random.RandomState(5)
    t = torch.from_numpy((rng.standard_normal((2, 4, 300)) * 3).astype(np.float32)).cuda().to(BF16)
    s = torch.from_numpy((rng.standard_normal((2, 4, 300)) * 3).astype(np.float32)).cuda().to(BF16).requires_grad_(True)
    labels = torch.zeros((2, 4), dtype=torch.int64, device="cuda")
    loss = kd_loss(s, t, labels, 1.0)
    loss.backward()
    rloss, _, rgrad = DR.kd_ref(t.float().reshape(-1, 300).cpu().numpy(), s.detach().float().reshape(-1, 300).cpu().numpy(),
                                labels.reshape(-1).cpu().numpy(), 1.0)
    assert abs(float(loss.detach()) - rloss) <= 1e-5 + 1e-4 * rloss
    assert s.grad.dtype == BF16
    got = s.grad.double().reshape(-1, 300).cpu().numpy()
    assert (np.abs(got - rgrad) <= 2e-5 / 8 + 2.0 ** -8 * np.abs(rgrad)).all()


def test_kd_loss_argument_errors():
    from kwhisper import ops

    t = torch.zeros((4, 50), device="cuda")
    s = torch.zeros((4, 50), device="cuda")
    lab = torch.zeros((4,), dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        ops.kd_loss(t.cpu(), s.cpu(), lab.cpu(), 1.0)
    with pytest.raises(ValueError):
        ops.kd_loss(t, s.cpu(), lab, 1.0)
    with pytest.raises(ValueError):
        ops.kd_loss(t, torch.zeros((4, 49), device="cuda"), lab, 1.0)       # V mismatch
    with pytest.raises(ValueError):
        ops.kd_loss(t, torch.zeros((3, 50), device="cuda"), lab, 1.0)       # N mismatch
    with pytest.raises(ValueError):
        ops.kd_loss(t, s, lab[:3], 1.0)                                     # N mismatch (labels)
    with pytest.raises(ValueError, match="alias"):
        ops.kd_loss(t, s, lab, 1.0, grad=s)                                 # grad aliasing student
    with pytest.raises(ValueError, match="alias"):
        ops.kd_loss(t, s, lab, 1.0, grad=t)                                 # grad aliasing teacher
    with pytest.raises(ValueError, match="temperature"):
        ops.kd_loss(t, s, lab, 0.0)
    with pytest.raises(ValueError):
        ops.kd_loss(t, s.to(torch.float16), lab, 1.0)
    old = ops.set_backend("ctypes")
    try:
        with pytest.raises(ValueError, match="alias"):
            ops.kd_loss(t, s, lab, 1.0, grad=s)
    finally:
        ops.set_backend(old)
