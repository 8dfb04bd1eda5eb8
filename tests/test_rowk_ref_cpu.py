"""tests/_rowk_ref.py checked on the host: the float32 emulation of layernorm_kernel / layernorm_bf16res_kernel lies
inside ``ln_bound`` on every family, dim, eps and output type of the GPU test, every mutant of the emulation leaves
the bound where the table below says it must, and a constant row gives beta bit for bit; and the argument checks of
kw_layernorm / kw_layernorm_bf16res, which return before any HIP call.  No kernel runs here."""
import ctypes
import functools

import numpy as np
import pytest

import _rowk_ref as K

F32, BF16 = K.F32, K.BF16
CASES = [(s, d) for s in (F32, BF16) for d in K.DIMS[s]]


@functools.lru_cache(maxsize=None)
def _case(stream, dim, with_delta):
    return K.ln_inputs(stream, dim, with_delta)


@functools.lru_cache(maxsize=None)
def _ref(stream, dim, with_delta, eps, out):
    c = _case(stream, dim, with_delta)
    return (K.ln_reference(c["post"], c["gamma"], c["beta"], eps),
            K.ln_bound(c["post"], c["gamma"], c["beta"], eps, out, stream))


def _emulate(stream, dim, with_delta, eps, out, **mutant):
    c = _case(stream, dim, with_delta)
    return K.emulate_ln_f32(c["x"], c["gamma"], c["beta"], eps, stream=stream, delta=c["delta"], out_dtype=out, **mutant)


def _ratios(stream, dim, with_delta, eps, out, **mutant):
    """family -> worst |emulation - reference| / bound over the family's rows."""
    ref, bound = _ref(stream, dim, with_delta, eps, out)
    r = K.ratio(_emulate(stream, dim, with_delta, eps, out, **mutant)[1], ref, bound)
    fam = _case(stream, dim, with_delta)["family"]
    return {name: float(r[fam == name].max()) for name in K.FAMILIES}


# ---------------------------------------------------------------------------------------------- the recipe
@pytest.mark.parametrize("stream,dim", CASES)
def test_recipe_properties(stream, dim):
    """What the bound and the GPU test rely on: every family present, the sums exact, x after the residual add a
    float32 / bf16 number that the emulation reproduces bit for bit, eps deciding the ``small`` row."""
    for with_delta in (False, True):
        c = _case(stream, dim, with_delta)
        fam = c["family"]
        assert [int((fam == n).sum()) for n in K.FAMILIES] == [5, 1, 1, 1, len(K.onehot_cols(dim))]
        assert len(fam) <= sum(K.ROW_COUNTS)
        assert sorted({i for w in K.row_windows(len(fam)) for i in w}) == list(range(len(fam)))  # every row launched
        assert K.sum_is_exact(c["post"]).all()
        assert np.array_equal(c["post"].astype(np.float32).astype(np.float64), c["post"])
        assert stream == F32 or K.is_bf16(c["post"])
        assert not K.is_bf16(c["beta"])
        x_after, _ = _emulate(stream, dim, with_delta, K.EPS[0], F32)
        assert np.array_equal(x_after.astype(np.float64), c["post"])
        var = c["post"][fam == "small"].var()
        assert 0 < var < K.EPS[0] / 1.5, var
    assert not K.sum_is_exact(np.full((1, 2048), 1.0 + 2.0 ** -20)).any()  # 2^31 units of 2^-20


@pytest.mark.parametrize("stream,dim", CASES)
def test_emulation_stays_inside_ln_bound(stream, dim):
    """A condition on the bound: the kernels' operation sequence in numpy float32 passes it on every row."""
    worst = {}
    for with_delta in (False, True):
        for eps in K.EPS:
            for out in (F32, BF16):
                for name, r in _ratios(stream, dim, with_delta, eps, out).items():
                    assert r <= 1.0, (stream, dim, with_delta, eps, out, name, r)
                    worst[out, name] = max(worst.get((out, name), 0.0), r)
    print(stream, dim, {f"{o}/{n}": round(r, 3) for (o, n), r in worst.items()})


@pytest.mark.parametrize("stream,dim", CASES)
def test_const_row_is_beta_bitwise(stream, dim):
    for with_delta in (False, True):
        c = _case(stream, dim, with_delta)
        row = c["family"] == "const"
        for eps in K.EPS:
            y32 = _emulate(stream, dim, with_delta, eps, F32)[1][row]
            y16 = _emulate(stream, dim, with_delta, eps, BF16)[1][row]
            assert np.array_equal(y32.view(np.uint32), c["beta"][None, :].view(np.uint32))
            assert np.array_equal(y16.view(np.uint32), K.rne_bf16(c["beta"])[None, :].view(np.uint32))


# ---------------------------------------------------------------------------------------------- the mutants
def _all_dims(stream, dim):
    return True


def _ragged_dims(stream, dim):  # (where dim is a multiple of 256 the padded divisor is dim itself)
    return dim % 256 != 0


def _wide_dims(stream, dim):
    return dim >= 252


# mutant -> (family that catches it, streams, output types, needs delta, dims); each entry is asserted for every dim
# it names, both eps and, unless it needs delta, with and without delta
CAUGHT_BY = {
    # at offset 1024 the one-pass variance has lost seven digits.  (bf16 numbers have eight bits: no row of them has a
    # mean above 2^7 spacings, the one-pass form loses three digits there and its two or three roundings can land
    # inside the bound -- the bf16 stream's offset row is not claimed.)
    "one_pass": [("offset", (F32,), (F32, BF16), False, _all_dims)],
    "drop_eps": [("small", (F32, BF16), (F32, BF16), False, _all_dims)],
    "eps_outside": [("small", (F32, BF16), (F32, BF16), False, _all_dims)],
    "dim_minus_1": [("recipe", (F32, BF16), (F32, BF16), False, _all_dims)],
    "padded_dim": [("recipe", (F32, BF16), (F32,), False, _ragged_dims)],
    "swap_gamma": [("recipe", (F32, BF16), (F32, BF16), False, _all_dims),
                   ("onehot", (F32, BF16), (F32, BF16), False, _all_dims)],
    # any bf16 output: every family from 252 columns on; below that a row has as few as four results, and a cut can
    # agree with the rounding on all of them -- the three families with unrelated results are caught even there
    "bf16_truncate": [(n, (F32, BF16), (BF16,), False, _all_dims) for n in ("recipe", "offset", "onehot")]
    + [(n, (F32, BF16), (BF16,), False, _wide_dims) for n in ("const", "small")],
    "stats_before_delta": [("recipe", (F32, BF16), (F32, BF16), True, _all_dims)],
    "unrounded_residual": [("recipe", (BF16,), (F32, BF16), True, _all_dims)],
}


def test_mutant_table_is_complete():
    assert set(CAUGHT_BY) == set(K.MUTANTS)
    assert ("offset", (F32,), (F32, BF16), False, _all_dims) in CAUGHT_BY["one_pass"]
    assert CAUGHT_BY["drop_eps"][0][0] == CAUGHT_BY["eps_outside"][0][0] == "small"
    assert {e[0] for e in CAUGHT_BY["bf16_truncate"]} == set(K.FAMILIES)


@pytest.mark.parametrize("mutant", K.MUTANTS)
def test_ln_bound_has_teeth(mutant):
    """Each corruption of the emulation leaves the bound on at least one element of the family the table names."""
    n = 0
    for family, streams, outs, needs_delta, dims in CAUGHT_BY[mutant]:
        for stream in streams:
            for dim in K.DIMS[stream]:
                if not dims(stream, dim):
                    continue
                for with_delta in (True,) if needs_delta else (False, True):
                    for eps in K.EPS:
                        for out in outs:
                            r = _ratios(stream, dim, with_delta, eps, out, **{mutant: True})[family]
                            assert r > 1.0, f"'{mutant}' passes the bound: {family} {stream} stream dim {dim} " \
                                            f"delta {with_delta} eps {eps} {out} out, ratio {r:.3g}"
                            n += 1
    print(f"{mutant}: caught in {n} of {n} cases")


# ---------------------------------------------------------------------------------------------- the C ABI's checks
A = 0x10000  # a 16-byte aligned address that is never dereferenced: every call below returns from the host-side check
# name -> (entry point, rows, dim, y type (0 f32, 1 bf16), byte offsets of x, gamma, beta, y, delta (None: no delta))
ABI_REJECTS = {
    "f32: dim % 4": ("kw_layernorm", 1, 6, 0, (0, 0, 0, 0, None)),
    "f32: dim > 2048": ("kw_layernorm", 1, 2052, 0, (0, 0, 0, 0, None)),
    "f32: rows < 0": ("kw_layernorm", -1, 256, 0, (0, 0, 0, 0, None)),
    "f32: x + 4": ("kw_layernorm", 1, 256, 0, (4, 0, 0, 0, None)),
    "f32: x + 8": ("kw_layernorm", 1, 256, 0, (8, 0, 0, 0, None)),
    "f32: gamma + 4": ("kw_layernorm", 1, 256, 0, (0, 4, 0, 0, None)),
    "f32: gamma + 8": ("kw_layernorm", 1, 256, 1, (0, 8, 0, 0, None)),
    "f32: beta + 4": ("kw_layernorm", 1, 256, 0, (0, 0, 4, 0, None)),
    "f32: beta + 8": ("kw_layernorm", 1, 256, 1, (0, 0, 8, 0, None)),
    "f32: f32 y + 8": ("kw_layernorm", 1, 256, 0, (0, 0, 0, 8, None)),
    "f32: bf16 y + 4": ("kw_layernorm", 1, 256, 1, (0, 0, 0, 4, None)),
    "f32: bf16 y + 2": ("kw_layernorm", 1, 256, 1, (0, 0, 0, 2, None)),
    "f32: delta + 4": ("kw_layernorm", 1, 256, 0, (0, 0, 0, 0, 4)),
    "f32: delta + 2": ("kw_layernorm", 1, 256, 1, (0, 0, 0, 0, 2)),
    "f32: rows 0, x + 4": ("kw_layernorm", 0, 256, 0, (4, 0, 0, 0, None)),  # checked before the rows == 0 return
    "bf16: dim % 8": ("kw_layernorm_bf16res", 1, 12, 0, (0, 0, 0, 0, None)),
    "bf16: dim > 2048": ("kw_layernorm_bf16res", 1, 2056, 1, (0, 0, 0, 0, None)),
    "bf16: x + 8": ("kw_layernorm_bf16res", 1, 256, 1, (8, 0, 0, 0, None)),
    "bf16: gamma + 4": ("kw_layernorm_bf16res", 1, 256, 1, (0, 4, 0, 0, None)),
    "bf16: gamma + 8": ("kw_layernorm_bf16res", 1, 256, 0, (0, 8, 0, 0, None)),
    "bf16: beta + 4": ("kw_layernorm_bf16res", 1, 256, 1, (0, 0, 4, 0, None)),
    "bf16: beta + 8": ("kw_layernorm_bf16res", 1, 256, 0, (0, 0, 8, 0, None)),
    "bf16: y + 8": ("kw_layernorm_bf16res", 1, 256, 1, (0, 0, 0, 8, None)),
    "bf16: delta + 8": ("kw_layernorm_bf16res", 1, 256, 1, (0, 0, 0, 0, 8)),
}


@pytest.fixture(scope="module")
def lib():
    """libkwhisper.so, built first where it is missing (as tests/test_abi.py does)."""
    import os
    import subprocess

    from conftest import ROOT
    from kwhisper import _lib

    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "kotoba-whisper_amd", "csrc"), "-j8"], check=True)
    return _lib.load()


def _abi_call(lib, fn, rows, dim, y_dtype, offs):
    p = [None if o is None else ctypes.c_void_p(A + o) for o in offs]
    return getattr(lib, fn)(p[0], rows, dim, p[1], p[2], 1e-5, p[3], y_dtype, p[4], None)


@pytest.mark.parametrize("name", list(ABI_REJECTS))
def test_c_abi_rejects_before_any_launch(lib, name):
    """kw_layernorm / kw_layernorm_bf16res return KW_EINVAL, with their name in the message, for every dim and
    alignment they cannot serve (no HIP call is made: this runs without a GPU, on addresses that are never read)."""
    from kwhisper import _lib

    fn, rows, dim, y_dtype, offs = ABI_REJECTS[name]
    assert _abi_call(lib, fn, rows, dim, y_dtype, offs) == _lib.KW_EINVAL
    assert fn.encode() in lib.kw_last_error()


@pytest.mark.parametrize("fn,y_dtype,offs", [
    ("kw_layernorm", 0, (0, 0, 0, 0, None)), ("kw_layernorm", 1, (0, 0, 0, 8, 8)), ("kw_layernorm", 0, (0, 0, 0, 0, 24)),
    ("kw_layernorm_bf16res", 1, (0, 0, 0, 0, 0)), ("kw_layernorm_bf16res", 0, (0, 0, 0, 16, None))])
def test_c_abi_accepts_zero_rows(lib, fn, y_dtype, offs):
    """rows == 0 with servable arguments is KW_OK and launches nothing (the 8-byte aligned bf16 y and delta of the
    f32 stream included)."""
    from kwhisper import _lib

    assert _abi_call(lib, fn, 0, 256, y_dtype, offs) == _lib.KW_OK
