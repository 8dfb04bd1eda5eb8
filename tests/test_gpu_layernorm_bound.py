"""The stand-alone row kernels of csrc/norm.hip on the MI355X: ``kw_layernorm`` / ``kw_layernorm_bf16res`` against the
float64 LayerNorm within the derived bound of tests/_rowk_ref.py, their host-side argument checks, and ``kw_embed``
bit for bit at its seams.  Both backends (``ops.set_backend``: the ctypes binding and torch.ops.kw).

LayerNorm: every family of ``_rowk_ref.ln_inputs`` (recipe, offset, const, small, onehot) at the dims on both sides
of the lane / slot seams, eps 1e-5 and 2^-6, f32 and bf16 y, with and without delta, the rows launched 1, 3, 4, 5 and
9 at a time.  x, y and delta sit among NaN sentinels (in front, behind and in one extra row after ``rows``); each
launch runs twice into fresh images.  Asserted: the result within ``ln_bound`` of ``ln_reference`` on x after the
residual add; constant rows equal to beta bit for bit; x the exact sum (rounded to bf16 on the bf16 stream) with
delta and untouched without; delta, gamma, beta and every sentinel untouched; the two launches bit-identical.  The
worst error / bound ratio per kernel, output type and family is printed and, with KW_LAYERNORM_REPORT=<file>, written
there (profiles/layernorm_bound.md); it is recorded, not asserted.

No rejection test launches anything: each returns from the host-side check, and the outputs are sentinels after it.
"""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from kwhisper import _lib as L  # noqa: E402
from kwhisper import ops  # noqa: E402

import _rowk_ref as K  # noqa: E402
from _gemm_ref import SENTINEL, bits_of, guarded, to_device  # noqa: E402

F32, BF16 = K.F32, K.BF16
TORCH = {F32: torch.float32, BF16: torch.bfloat16}
FRONT = BACK = 64  # sentinel elements in front of and behind every image (a multiple of 16 bytes in both types)
_MEASURED = {}  # (kernel, family) -> [worst error / bound, rows]


def _kernel(stream, out):
    return f"{'layernorm_kernel' if stream == F32 else 'layernorm_bf16res_kernel'}<{'float' if out == F32 else 'bf16_t'}>"


@pytest.fixture(scope="module", autouse=True)
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()
    yield
    lines = ["| kernel | family | worst error / bound | rows checked |", "|---|---|---|---|"]
    for kernel in [_kernel(s, o) for s in (F32, BF16) for o in (F32, BF16)]:
        for family in K.FAMILIES:
            if (kernel, family) in _MEASURED:
                worst, rows = _MEASURED[kernel, family]
                lines.append(f"| `{kernel}` | {family} | {worst:.4f} | {rows} |")
    print("\n".join(lines))
    path = os.environ.get("KW_LAYERNORM_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")


@pytest.fixture(params=["ctypes", "torch"])
def backend(request):
    old = ops.set_backend(request.param)
    yield request.param
    ops.set_backend(old)


# ------------------------------------------------------------------------------------------------ images
def _image(values, dtype, extra_rows=1):
    """values [R, dim] float32 -> (flat guarded buffer, its [R, dim] view): FRONT sentinels, the rows, ``extra_rows``
    rows of sentinels and BACK more."""
    R, dim = values.shape
    buf = guarded(FRONT + (R + extra_rows) * dim + BACK, dtype, "cuda")
    view = buf[FRONT:FRONT + R * dim].view(R, dim)
    view.copy_(to_device(values, dtype, "cuda"))
    return buf, view


def _blank(R, dim, dtype):
    buf = guarded(FRONT + (R + 1) * dim + BACK, dtype, "cuda")
    return buf, buf[FRONT:FRONT + R * dim].view(R, dim)


def _bits(t) -> np.ndarray:
    return bits_of(t).cpu().numpy()


def _values(bits: np.ndarray, dtype) -> np.ndarray:
    """Bit patterns (int64) -> float64 values."""
    u = bits.astype(np.uint32) if dtype == torch.float32 else bits.astype(np.uint32) << 16
    return u.view(np.float32).astype(np.float64)


def _want_bits(values, dtype) -> np.ndarray:
    return _bits(to_device(np.ascontiguousarray(values, dtype=np.float32), dtype, "cpu"))


def _outside_intact(bits, R, dim, dtype) -> bool:
    s = SENTINEL[dtype]
    return bool((bits[:FRONT] == s).all() and (bits[FRONT + R * dim:] == s).all())


# ------------------------------------------------------------------------------------------------ LayerNorm
@functools.lru_cache(maxsize=None)
def _case(stream, dim, with_delta):
    return K.ln_inputs(stream, dim, with_delta)


@functools.lru_cache(maxsize=None)
def _ref(stream, dim, with_delta, eps, out):
    """(reference, bound) of the whole pool of rows, computed once and shared by both backends."""
    c = _case(stream, dim, with_delta)
    return (K.ln_reference(c["post"], c["gamma"], c["beta"], eps),
            K.ln_bound(c["post"], c["gamma"], c["beta"], eps, out, stream))


LN_CASES = [(s, d, wd) for s in (F32, BF16) for d in K.DIMS[s] for wd in (False, True)]


@pytest.mark.parametrize("stream,dim,with_delta", LN_CASES)
def test_layernorm_within_derived_bound(backend, stream, dim, with_delta):
    c = _case(stream, dim, with_delta)
    xt = TORCH[stream]
    g = torch.from_numpy(c["gamma"]).cuda()
    b = torch.from_numpy(c["beta"]).cuda()
    g0, b0 = g.clone(), b.clone()
    beta_bits = {F32: _want_bits(c["beta"], torch.float32), BF16: _want_bits(c["beta"], torch.bfloat16)}
    worst = {}
    for eps in K.EPS:
        for out in (F32, BF16):
            yt = TORCH[out]
            ref, bound = _ref(stream, dim, with_delta, eps, out)
            for rows in K.row_windows(len(c["family"])):
                R = len(rows)
                what = f"{_kernel(stream, out)} dim {dim} delta {with_delta} eps {eps:g} rows {rows}"
                images = []
                for _ in range(2):
                    xbuf, x = _image(c["x"][rows], xt)
                    dbuf, d = _image(c["delta"][rows], torch.bfloat16) if with_delta else (None, None)
                    d_before = _bits(dbuf) if with_delta else None
                    ybuf, y = _blank(R, dim, yt)
                    ops.layernorm(x, g, b, eps, y, delta=d)
                    images.append((_bits(xbuf), _bits(ybuf)))
                    if with_delta:
                        assert np.array_equal(_bits(dbuf), d_before), f"{what}: delta was written"
                xb, yb = images[0]
                assert np.array_equal(xb, images[1][0]) and np.array_equal(yb, images[1][1]), f"{what}: not repeatable"
                assert _outside_intact(xb, R, dim, xt), f"{what}: sentinels around x overwritten"
                assert _outside_intact(yb, R, dim, yt), f"{what}: sentinels around y overwritten"
                # x: the exact sum (its bf16 rounding) with delta, its input without
                got_x = xb[FRONT:FRONT + R * dim].reshape(R, dim)
                assert np.array_equal(got_x, _want_bits(c["post"][rows], xt).reshape(R, dim)), f"{what}: x after the launch"
                # y: inside the bound, constant rows beta itself
                got_bits = yb[FRONT:FRONT + R * dim].reshape(R, dim)
                q = K.ratio(_values(got_bits.reshape(-1), yt).reshape(R, dim), ref[rows], bound[rows])
                fam = c["family"][rows]
                for name in set(fam):
                    r = float(q[fam == name].max())
                    worst[out, name] = max(worst.get((out, name), 0.0), r)
                    rec = _MEASURED.setdefault((_kernel(stream, out), name), [0.0, 0])
                    rec[0], rec[1] = max(rec[0], r), rec[1] + int((fam == name).sum())
                bad = np.argwhere(q > 1.0)
                assert bad.size == 0, f"{what}: {len(bad)} results outside ln_bound, worst ratio {float(q.max()):.3f} at " \
                                      f"(row, col) {tuple(bad[0])} of family {fam[bad[0][0]]}"
                for m in np.nonzero(fam == "const")[0]:
                    assert np.array_equal(got_bits[m], beta_bits[out]), f"{what}: constant row {m} is not beta bit for bit"
    assert torch.equal(g, g0) and torch.equal(b, b0)
    print(stream, dim, with_delta, backend, {f"{o}/{n}": round(r, 3) for (o, n), r in sorted(worst.items())})


# ------------------------------------------------------------------------------------------------ host checks
def _ramp(n, period, step, lo, dtype):
    """lo, lo + step, ... repeating every ``period`` elements: multiples of 1/4, exact in either type."""
    return ((torch.arange(n, device="cuda") % period) * step + lo).to(dtype)


def _run_plain(backend, stream, dim, out, x_off=0, y_off=0, d_off=None, g_off=0, b_off=0, *, rows=3, gamma=None,
               beta=None, y_dtype=None, y_elems=None, d_dtype=torch.bfloat16, d_elems=None):
    """One LayerNorm call whose tensors are views ``*_off`` elements past a 256-byte boundary of their buffers (or
    of another size / type): returns (call, ybuf, xbuf).  The ctypes backend goes through ops.layernorm (its checks,
    then the C ABI's); the torch backend calls torch.ops.kw.layernorm itself, where ops.layernorm hands everything
    on that backend: the checks met are those of torch_ops.cpp, then the C ABI's."""
    xt, yt = TORCH[stream], y_dtype or TORCH[out]
    n = rows * dim
    xbuf = guarded(FRONT + n + BACK, xt, "cuda")
    x = xbuf[FRONT + x_off:FRONT + x_off + n].view(rows, dim)
    x.copy_(_ramp(n, 17, 0.25, -2.0, xt).view(rows, dim))
    ye = n if y_elems is None else y_elems
    ybuf = guarded(FRONT + n + BACK, yt, "cuda") if yt in SENTINEL else torch.zeros(FRONT + n + BACK, dtype=yt, device="cuda")
    y = ybuf[FRONT + y_off:FRONT + y_off + ye]
    y = y.view(rows, dim) if ye == n else y
    gb, bb = torch.ones(dim + 8, device="cuda"), torch.zeros(dim + 8, device="cuda")
    gb[g_off:g_off + dim] = _ramp(dim, 5, 0.25, 0.5, torch.float32)  # the same values at any offset
    bb[b_off:b_off + dim] = _ramp(dim, 3, 0.5, -0.5, torch.float32)
    g = gb[g_off:g_off + dim] if gamma is None else gamma
    b = bb[b_off:b_off + dim] if beta is None else beta
    d = None
    if d_off is not None:
        de = n if d_elems is None else d_elems
        dbuf = torch.zeros(FRONT + 16 + n + BACK, dtype=d_dtype, device="cuda")
        dbuf[FRONT + d_off:FRONT + d_off + n] = _ramp(n, 7, 0.25, -0.75, d_dtype)
        d = dbuf[FRONT + d_off:FRONT + d_off + de]
        d = d.view(rows, dim) if de == n else d
    if backend == "torch":
        assert ops.backend() == "torch"
        return (lambda: L.load_torch_ops().layernorm(x, g, b, 1e-5, y, d)), ybuf, xbuf
    assert ops.backend() == "ctypes"
    return (lambda: ops.layernorm(x, g, b, 1e-5, y, delta=d)), ybuf, xbuf


def _untouched(buf) -> bool:
    if buf.dtype not in SENTINEL:
        return bool((buf == 0).all())
    return bool((bits_of(buf) == SENTINEL[buf.dtype]).all())


# (stream, dim, y type, keyword arguments of _run_plain): each must raise ValueError before any launch
_G = lambda n, dt=torch.float32: torch.ones(n, device="cuda", dtype=dt)  # noqa: E731
REJECTS = {
    "f32 dim % 4": (F32, 6, F32, {}),
    "bf16 dim % 8": (BF16, 12, F32, {}),
    "f32 dim > 2048": (F32, 2052, F32, {}),
    "bf16 dim > 2048": (BF16, 2056, BF16, {}),
    # gamma / beta: contiguous f32 of exactly dim elements
    "gamma short": (F32, 256, F32, dict(gamma=lambda: _G(252))),
    "gamma long": (F32, 256, F32, dict(gamma=lambda: _G(260))),
    "gamma bf16": (F32, 256, F32, dict(gamma=lambda: _G(256, torch.bfloat16))),
    "gamma strided": (F32, 256, F32, dict(gamma=lambda: _G(512)[::2])),
    "beta short": (BF16, 256, BF16, dict(beta=lambda: _G(248))),
    "beta f64": (BF16, 256, BF16, dict(beta=lambda: _G(256, torch.float64))),
    "beta strided": (BF16, 256, BF16, dict(beta=lambda: _G(512)[::2])),
    # out: contiguous f32 / bf16 of x's element count
    "out short": (F32, 256, F32, dict(y_elems=2 * 256)),
    "out f16": (F32, 256, F32, dict(y_dtype=torch.float16)),
    "out short bf16 stream": (BF16, 256, BF16, dict(y_elems=3 * 256 - 8)),
    # delta: bf16 of x's size
    "delta f32": (F32, 256, F32, dict(d_off=0, d_dtype=torch.float32)),
    "delta short": (F32, 256, BF16, dict(d_off=0, d_elems=2 * 256)),
    "delta short bf16 stream": (BF16, 256, BF16, dict(d_off=0, d_elems=2 * 256)),
    # alignment, f32 stream: x, gamma, beta, f32 y 16 bytes; bf16 y and delta 8 bytes
    "f32 x + 4 B": (F32, 256, F32, dict(x_off=1)),
    "f32 x + 8 B": (F32, 256, F32, dict(x_off=2)),
    "f32 gamma + 4 B": (F32, 256, F32, dict(g_off=1)),
    "f32 gamma + 8 B": (F32, 256, BF16, dict(g_off=2)),
    "f32 beta + 4 B": (F32, 256, F32, dict(b_off=1)),
    "f32 beta + 8 B": (F32, 256, BF16, dict(b_off=2)),
    "f32 y(f32) + 4 B": (F32, 256, F32, dict(y_off=1)),
    "f32 y(f32) + 8 B": (F32, 256, F32, dict(y_off=2)),
    "f32 y(bf16) + 2 B": (F32, 256, BF16, dict(y_off=1)),
    "f32 y(bf16) + 4 B": (F32, 256, BF16, dict(y_off=2)),
    "f32 delta + 2 B": (F32, 256, F32, dict(d_off=1)),
    "f32 delta + 4 B": (F32, 256, F32, dict(d_off=2)),
    # alignment, bf16 stream: everything 16 bytes
    "bf16 x + 8 B": (BF16, 256, BF16, dict(x_off=4)),
    "bf16 x + 2 B": (BF16, 256, F32, dict(x_off=1)),
    "bf16 y(bf16) + 8 B": (BF16, 256, BF16, dict(y_off=4)),
    "bf16 y(f32) + 8 B": (BF16, 256, F32, dict(y_off=2)),
    "bf16 delta + 8 B": (BF16, 256, BF16, dict(d_off=4)),
    "bf16 gamma + 4 B": (BF16, 256, BF16, dict(g_off=1)),
    "bf16 gamma + 8 B": (BF16, 256, F32, dict(g_off=2)),
    "bf16 beta + 4 B": (BF16, 256, BF16, dict(b_off=1)),
    "bf16 beta + 8 B": (BF16, 256, F32, dict(b_off=2)),
}


@pytest.mark.parametrize("name", list(REJECTS))
def test_layernorm_rejects(backend, name):
    """Each bad argument is refused with ValueError by the host-side checks (ops.layernorm, torch.ops.kw.layernorm,
    kw_layernorm / kw_layernorm_bf16res), and neither y nor x has been written."""
    stream, dim, out, kw = REJECTS[name]
    kw = {k: (v() if callable(v) else v) for k, v in kw.items()}
    call, ybuf, xbuf = _run_plain(backend, stream, dim, out, **kw)
    x_before = bits_of(xbuf).clone()
    with pytest.raises(ValueError):
        call()
    torch.cuda.synchronize()
    assert _untouched(ybuf), f"{name}: y was written"
    assert torch.equal(bits_of(xbuf), x_before), f"{name}: x was written"


@pytest.mark.parametrize("stream,out,kw", [(F32, BF16, dict(y_off=4)), (F32, F32, dict(d_off=4)),
                                           (F32, BF16, dict(y_off=4, d_off=12))])
def test_layernorm_accepts_8_byte_aligned_bf16_operands(backend, stream, out, kw):
    """The f32 stream's kernel moves a bf16 y and delta 8 bytes at a time: views 8 bytes past a 16-byte boundary are
    valid and give the aligned launch's result bit for bit."""
    call, ybuf, xbuf = _run_plain(backend, stream, 260, out, **kw)
    call()
    ref_call, ref_ybuf, ref_xbuf = _run_plain(backend, stream, 260, out, d_off=0 if "d_off" in kw else None)
    ref_call()
    off, n = kw.get("y_off", 0), 3 * 260
    assert torch.equal(bits_of(ybuf)[FRONT + off:FRONT + off + n], bits_of(ref_ybuf)[FRONT:FRONT + n])
    assert torch.equal(bits_of(xbuf), bits_of(ref_xbuf))
    s = SENTINEL[ybuf.dtype]
    assert bool((bits_of(ybuf)[:FRONT + off] == s).all() and (bits_of(ybuf)[FRONT + off + n:] == s).all())
    assert not bool((bits_of(ybuf)[FRONT + off:FRONT + off + n] == s).any())


@pytest.mark.parametrize("stream,out", [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)])
def test_layernorm_zero_rows(backend, stream, out):
    """rows = 0 is valid and writes nothing, through ops.layernorm on either backend and at the C ABI."""
    dim = 256
    xbuf, x = _blank(0, dim, TORCH[stream])
    ybuf, y = _blank(0, dim, TORCH[out])
    g, b = torch.ones(dim, device="cuda"), torch.zeros(dim, device="cuda")
    ops.layernorm(x, g, b, 1e-5, y)
    fn = L.load().kw_layernorm if stream == F32 else L.load().kw_layernorm_bf16res
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    e = xbuf.element_size()
    rc = fn(p(xbuf, FRONT * e), 0, dim, p(g), p(b), 1e-5, p(ybuf, FRONT * ybuf.element_size()), L.KW_DT_F32 if out == F32
            else L.KW_DT_BF16, None, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == L.KW_OK
    torch.cuda.synchronize()
    assert _untouched(xbuf) and _untouched(ybuf)


# ------------------------------------------------------------------------------------------------ kw_embed
V_FULL, N_POS = 51866, 448


@functools.lru_cache(maxsize=None)
def _tables(V, d, dtype):
    g = torch.Generator(device="cuda").manual_seed(V + d)
    tok = torch.randn(V, d, device="cuda", generator=g).to(dtype)
    pos = torch.randn(N_POS, d, device="cuda", generator=g).to(dtype)
    return tok, pos


def _embed_case(tok, pos, ids, B, q, cur, hb_off=0):
    """Launch kw_embed with h and hb among sentinels (hb ``hb_off`` elements past its 16-byte boundary); assert both
    bit for bit against the float64 sum rounded once to f32 (and from there to bf16), and the sentinels.  Returns
    (h bits, hb bits) of the images."""
    d = tok.shape[1]
    n = B * q * d
    hbuf = guarded(FRONT + n + BACK, torch.float32, "cuda")
    hbbuf = guarded(FRONT + hb_off + n + BACK, torch.bfloat16, "cuda")
    h = hbuf[FRONT:FRONT + n].view(B * q, d)
    hb = hbbuf[FRONT + hb_off:FRONT + hb_off + n].view(B * q, d)
    cur_t = torch.tensor([cur], dtype=torch.int32, device="cuda")
    ids0 = ids.clone()
    ops.embed(ids, B, q, cur_t, tok, pos, h, hb)
    p = torch.arange(cur - q, cur, device="cuda")
    want = (tok[ids[:, cur - q:cur]].double() + pos[p].double()[None]).reshape(B * q, d).float()  # one rounding
    hbits, hbbits = bits_of(hbuf), bits_of(hbbuf)
    lo, lob = FRONT, FRONT + hb_off
    assert torch.equal(hbits[lo:lo + n], bits_of(want).reshape(-1))
    assert torch.equal(hbbits[lob:lob + n], bits_of(want.bfloat16()).reshape(-1))
    assert bool((hbits[:lo] == SENTINEL[torch.float32]).all() and (hbits[lo + n:] == SENTINEL[torch.float32]).all())
    assert bool((hbbits[:lob] == SENTINEL[torch.bfloat16]).all() and (hbbits[lob + n:] == SENTINEL[torch.bfloat16]).all())
    assert torch.equal(ids, ids0) and int(cur_t) == cur
    return hbits[lo:lo + n], hbbits[lob:lob + n]


def _ids(B, width, V, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, V, (B, width), device="cuda", generator=g)


@pytest.mark.parametrize("q,cur", [(1, 1), (2, 2), (4, 4), (1, 448), (3, 448), (2, 7)])
def test_embed_first_and_last_position(backend, q, cur):
    """cur_len == q_len reads position 0; cur_len 448 reads the last row of pos_emb (and the last id of the row)."""
    tok, pos = _tables(1000, 384, torch.bfloat16)
    _embed_case(tok, pos, _ids(3, N_POS, 1000, q + cur), 3, q, cur)


def test_embed_first_and_last_id_of_the_full_vocabulary(backend):
    tok, pos = _tables(V_FULL, 1280, torch.bfloat16)
    ids = _ids(4, N_POS, V_FULL, 5)
    ids[:, 5] = torch.tensor([0, V_FULL - 1, V_FULL - 1, 0], device="cuda")
    ids[:, 6] = torch.tensor([V_FULL - 1, 0, 1, V_FULL - 2], device="cuda")
    _embed_case(tok, pos, ids, 4, 2, 7)


@pytest.mark.parametrize("q,cur", [(1, 9), (3, 9), (9, 9)])
def test_embed_ids_stride_larger_than_cur_len(backend, q, cur):
    """ids is a [B, cur_len] view of a wider buffer (row stride 61, first column 5): other ids lie on every side."""
    tok, pos = _tables(1000, 384, torch.bfloat16)
    wide = _ids(3, 61, 1000, 17)
    ids = wide[:, 5:5 + cur]
    assert ids.stride(0) == 61 > cur
    _embed_case(tok, pos, ids, 3, q, cur)


@pytest.mark.parametrize("d", [384, 12])
@pytest.mark.parametrize("q,cur", [(1, 1), (2, 7), (1, 448)])
def test_embed_f32_tables(backend, d, q, cur):
    """embed_kernel<float>: f32 tables, the f32 sum and its bf16 mirror."""
    tok, pos = _tables(1000, d, torch.float32)
    _embed_case(tok, pos, _ids(3, N_POS, 1000, d + q), 3, q, cur)


@pytest.mark.parametrize("d", [8, 384, 1280])
def test_embed_misaligned_mirror_takes_the_element_kernel(backend, d):
    """bf16 tables, d % 8 == 0, hb 8 bytes past a 16-byte boundary: the element kernel runs in place of the 16-byte
    vector kernel and gives its result bit for bit."""
    tok, pos = _tables(1000, d, torch.bfloat16)
    ids = _ids(5, N_POS, 1000, d)
    vec = _embed_case(tok, pos, ids, 5, 2, 7)
    elem = _embed_case(tok, pos, ids, 5, 2, 7, hb_off=4)
    assert torch.equal(vec[0], elem[0]) and torch.equal(vec[1], elem[1])
