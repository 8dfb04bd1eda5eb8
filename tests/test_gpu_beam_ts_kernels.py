"""The two kernels behind token timestamps under beam search, on the MI355X: kw_align_weights_rows against
kw_align_weights (on a log gathered on the host, and on every running row with the gather after it, as the
reference does), and kw_beam_select_parents against kw_beam_select and the step
restatement with the parent outputs (tests/_beam_ts_ref.py).  Every comparison is exact (bitwise for floats)."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _beam_ref as R  # noqa: E402
import _beam_ts_ref as T  # noqa: E402
from kwhisper import _lib as L  # noqa: E402
from kwhisper import ops  # noqa: E402

F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()


@pytest.fixture(params=["torch", "ctypes"])
def backend(request):
    old = ops.set_backend(request.param)
    yield request.param
    ops.set_backend(old)


def _bits(x):
    return x.view(torch.int32)


# ---- kw_align_weights_rows -----------------------------------------------------------------------------------
def _log_and_keys(rng, dtype, A, R_, t_log, B, H, S):
    log = torch.from_numpy((0.6 * rng.standard_normal((A, R_, t_log, 64))).astype(F32)).to(dtype).cuda()
    k = torch.from_numpy(rng.standard_normal((1, B, H, S, 64)).astype(F32)).to(dtype).cuda()
    return log, k


def _gathered(log, rows):
    """log [A][R][t_log][64], rows (B, T) -> [A][B][t_log][64] with step t of item b taken from row rows[b][t]."""
    A, _, t_log, _ = log.shape
    B, T_ = rows.shape
    out = torch.zeros((A, B, t_log, 64), dtype=log.dtype, device=log.device)
    for b in range(B):
        for t in range(T_):
            out[:, b, t] = log[:, int(rows[b, t]), t]
    return out


def _both(log, rows, k, pairs, T_, S, rows_for_gather=None):
    """(kw_align_weights_rows through the table; the reference's order: kw_align_weights of every running row over
    its own item's keys, then the gather by the table), both as flat arrays; a canary behind the first."""
    A, B, R_ = len(pairs), k.shape[1], log.shape[1]
    got = torch.full((A * B * T_ * S + 64,), -7.0, device="cuda")
    ops.align_weights_rows(log, torch.from_numpy(rows.astype(np.int32)).cuda(), k, pairs, T_, got)
    full = torch.empty((A, R_, T_, S), device="cuda")
    ops.align_weights(log, k.repeat_interleave(R_ // B, dim=1).contiguous(), pairs, T_, full)
    rg = rows if rows_for_gather is None else rows_for_gather
    want = torch.stack([torch.stack([full[:, int(rg[b, t]), t] for t in range(T_)], 1) for b in range(B)], 1)
    torch.cuda.synchronize()
    assert (got[-64:] == -7.0).all()
    got = got[:-64]
    assert not torch.isnan(got).any() and float(got.min()) >= 0.0
    return got, want.contiguous().reshape(-1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_align_weights_rows_equals_align_weights_on_a_gathered_log(dtype, backend):
    """A = 2, R = 6 (2 items x 3 beams), T = 19 (a full 16-step block and a ragged 3), S = 100 (no multiple of 16)."""
    rng = np.random.default_rng(7)
    A, R_, B, H, S, T_, t_log = 2, 6, 2, 3, 100, 19, 24
    pairs = [(0, 0), (0, 2)]
    log, k = _log_and_keys(rng, dtype, A, R_, t_log, B, H, S)
    # a table as a search leaves it: every item's steps in its own running rows, switching between them
    rows = rng.integers(0, R_ // B, (B, T_)) + (R_ // B) * np.arange(B)[:, None]
    assert len(set(rows[0, :16].tolist())) > 1 and len(set(rows[1, 16:].tolist())) > 1
    got, want = _both(log, rows, k, pairs, T_, S)
    assert torch.equal(_bits(got), _bits(want))
    gathered = torch.empty((len(pairs), B, T_, S), device="cuda")
    ops.align_weights(_gathered(log, rows), k, pairs, T_, gathered)  # item b's keys: the rows are b's own
    assert torch.equal(_bits(got), _bits(gathered.reshape(-1)))
    # the table matters: the item's own first row instead gives other weights
    plain = torch.empty_like(gathered)
    ops.align_weights(_gathered(log, np.tile(np.array([[0], [3]]), (1, T_))), k, pairs, T_, plain)
    assert not torch.equal(_bits(plain), _bits(gathered))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_align_weights_rows_takes_the_keys_of_the_rows_item(dtype, backend):
    """A hypothesis shorter than the pass's longest reads running row 0 -- a row of item 0, which attends item 0's
    keys -- for its remaining steps; and any table at all: rows of both items mixed inside one 16-step block."""
    rng = np.random.default_rng(11)
    A, R_, B, H, S, T_, t_log = 2, 6, 2, 3, 100, 19, 24
    pairs = [(0, 0), (0, 2)]
    log, k = _log_and_keys(rng, dtype, A, R_, t_log, B, H, S)
    rows = rng.integers(0, R_ // B, (B, T_)) + (R_ // B) * np.arange(B)[:, None]
    rows[1, 9:] = 0  # item 1's hypothesis ends inside the first block
    got, want = _both(log, rows, k, pairs, T_, S)
    assert torch.equal(_bits(got), _bits(want))
    other = torch.empty((len(pairs), B, T_, S), device="cuda")
    ops.align_weights(_gathered(log, rows), k, pairs, T_, other)  # row 0's queries over item 1's keys: not the same
    assert not torch.equal(_bits(got), _bits(other.reshape(-1)))
    rows = rng.integers(0, R_, (B, T_))
    assert len({int(r) // 3 for r in rows[0, :16]}) == 2
    got, want = _both(log, rows, k, pairs, T_, S)
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_align_weights_rows_identity_table(dtype, backend):
    """R = B and rows[b][t] = b: kw_align_weights on the log itself."""
    rng = np.random.default_rng(8)
    A, B, H, S, T_, t_log = 2, 6, 3, 100, 19, 19
    pairs = [(0, 1), (0, 2)]
    log, k = _log_and_keys(rng, dtype, A, B, t_log, B, H, S)
    rows = np.tile(np.arange(B)[:, None], (1, T_))
    got = torch.empty((A, B, T_, S), device="cuda")
    want = torch.empty((A, B, T_, S), device="cuda")
    ops.align_weights_rows(log, torch.from_numpy(rows.astype(np.int32)).cuda(), k, pairs, T_, got)
    ops.align_weights(log, k, pairs, T_, want)
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_align_weights_rows_one_step_whole_encoder(dtype, backend):
    """S = 1500, T = 1 (a two-token hypothesis)."""
    rng = np.random.default_rng(9)
    A, R_, B, H, S, T_, t_log = 2, 6, 2, 3, 1500, 1, 5
    pairs = [(0, 0), (0, 1)]
    log, k = _log_and_keys(rng, dtype, A, R_, t_log, B, H, S)
    got, want = _both(log, np.array([[2], [0]]), k, pairs, T_, S)
    assert torch.equal(_bits(got), _bits(want))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_align_weights_rows_clamps_entries_outside_the_log(dtype, backend):
    """Entries outside [0, R) are read as the nearest row of the log (include/kwhisper.h): the result is that of the
    clamped table, the log is not left.  Bad arguments come back as KW_EINVAL (ValueError)."""
    rng = np.random.default_rng(10)
    A, R_, B, H, S, T_, t_log = 2, 6, 2, 3, 100, 19, 19
    pairs = [(0, 0), (0, 2)]
    log, k = _log_and_keys(rng, dtype, A, R_, t_log, B, H, S)
    rows = rng.integers(0, R_, (B, T_)).astype(np.int64)
    rows[0, [0, 5, 17]] = [-1, R_, 2 ** 31 - 1]
    rows[1, [3, 16, 18]] = [-(2 ** 31), 1 << 20, R_ + 1]
    got, want = _both(log, rows, k, pairs, T_, S, rows_for_gather=np.clip(rows, 0, R_ - 1))
    assert torch.equal(_bits(got), _bits(want))
    out = torch.empty((A, B, T_, S), device="cuda")
    table = torch.zeros((B, T_), dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):  # T beyond the log
        ops.align_weights_rows(log, torch.zeros((B, t_log + 1), dtype=torch.int32, device="cuda"), k, pairs, t_log + 1,
                               torch.empty((A, B, t_log + 1, S), device="cuda"))
    with pytest.raises(ValueError):  # a head outside the cache
        ops.align_weights_rows(log, table, k, [(0, 0), (0, H)], T_, out)
    with pytest.raises(ValueError):  # a table of another shape
        ops.align_weights_rows(log, table[:, :-1].contiguous(), k, pairs, T_, out)
    with pytest.raises(ValueError):  # log rows that are no whole number of rows per item
        ops.align_weights_rows(log[:, :5].contiguous(), table, k, pairs, T_, out)
    lib = L.load()
    rc = lib.kw_align_weights_rows(L.KW_DT_F32, None, R_, t_log, None, None, 0, 1, None, A, B, H, S, T_, None, None)
    assert rc == L.KW_EINVAL and b"kw_align_weights_rows" in lib.kw_last_error()


# ---- kw_beam_select_parents ----------------------------------------------------------------------------------
SEL_KEYS = ("ids", "bp", "run_scores", "fin_seq", "fin_score", "fin_len", "fin_flag", "unsat", "cur_len", "counter", "go",
            "done", "item_flags")


class _State:
    """The device state of a search from its first step (oracle.generate.beam_init), and kw_beam_select's arguments."""

    def __init__(self, prompt, nb, V, max_length, eos, fill, length_penalty, early_stopping):
        B, P = prompt.shape
        Rn = B * nb
        i32, dev = torch.int32, "cuda"
        ids = torch.zeros((Rn, max_length + 2), dtype=torch.int64, device=dev)
        ids[:, :P] = torch.from_numpy(np.repeat(prompt, nb, 0)).to(dev)
        rs = torch.full((B, nb), -1.0e9, device=dev)
        rs[:, 0] = 0.0
        self.t = t = dict(
            ids=ids, bp=torch.arange(Rn, dtype=i32, device=dev)[:, None].expand(Rn, max_length).contiguous(),
            run_scores=rs.reshape(-1).contiguous(), fin_seq=torch.full((B, nb, max_length), fill, dtype=torch.int64, device=dev),
            fin_score=torch.full((B, nb), -1.0e9, device=dev), fin_len=torch.zeros((B, nb), dtype=i32, device=dev),
            fin_flag=torch.zeros((B, nb), dtype=i32, device=dev), unsat=torch.ones((B,), dtype=i32, device=dev),
            cur_len=torch.full((1,), P, dtype=i32, device=dev), counter=torch.zeros(1, dtype=i32, device=dev),
            go=torch.ones(1, dtype=i32, device=dev), done=torch.zeros(1, dtype=i32, device=dev),
            item_flags=torch.zeros((B, 3), dtype=i32, device=dev), cand_val=torch.zeros((Rn, 2 * nb), device=dev),
            cand_idx=torch.zeros((Rn, 2 * nb), dtype=i32, device=dev),
            parent_log=torch.full((max_length, Rn), -5, dtype=i32, device=dev),
            fin_parent=torch.full((B, nb), -1, dtype=i32, device=dev))
        es = 2 if early_stopping == "never" else int(bool(early_stopping))
        self.cfg = [B, nb, V, P, max_length, eos, fill, es]
        self.lp = float(length_penalty)
        b = self.b = L.BeamSelectArgs()
        b.B, b.num_beams, b.V = B, nb, V
        b.cand_val, b.cand_idx = t["cand_val"].data_ptr(), t["cand_idx"].data_ptr()
        b.ids, b.ids_stride = t["ids"].data_ptr(), t["ids"].stride(0)
        b.bp, b.bp_stride = t["bp"].data_ptr(), t["bp"].stride(0)
        b.run_scores = t["run_scores"].data_ptr()
        b.fin_seq, b.fin_stride = t["fin_seq"].data_ptr(), t["fin_seq"].shape[-1]
        b.fin_score, b.fin_len, b.fin_flag = t["fin_score"].data_ptr(), t["fin_len"].data_ptr(), t["fin_flag"].data_ptr()
        b.unsat, b.cur_len = t["unsat"].data_ptr(), t["cur_len"].data_ptr()
        b.begin_index, b.max_length, b.eos_id, b.fill_id = P, max_length, eos, fill
        b.length_penalty, b.early_stopping = self.lp, es
        b.counter, b.go, b.done = t["counter"].data_ptr(), t["go"].data_ptr(), t["done"].data_ptr()
        b.item_flags = t["item_flags"].data_ptr()

    def select(self, backend, parents):
        t = self.t
        sel = (t["cand_val"], t["cand_idx"], t["ids"], t["bp"], t["run_scores"], t["fin_seq"], t["fin_score"], t["fin_len"],
               t["fin_flag"], t["unsat"], t["cur_len"], t["counter"], t["go"], t["done"], t["item_flags"], self.cfg, self.lp)
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if backend == "torch":
            kw = L.load_torch_ops()
            if parents:
                kw.beam_select_parents(*sel, t["parent_log"], t["fin_parent"])
            else:
                kw.beam_select(*sel)
        elif parents:
            L.check(L.load().kw_beam_select_parents(ctypes.byref(self.b), ctypes.c_void_p(t["parent_log"].data_ptr()),
                                                    ctypes.c_void_p(t["fin_parent"].data_ptr()), stream),
                    "kw_beam_select_parents")
        else:
            L.check(L.load().kw_beam_select(ctypes.byref(self.b), stream), "kw_beam_select")


def select_case():
    """B = 2, 3 beams, V = 64, EOS near the top of most rows.  With this seed the search runs all five steps, both
    items finish, a finished entry changes its slot and one hypothesis is taken from a row that is not its item's
    first (asserted below on the restatement)."""
    return dict(B=2, nb=3, V=64, P=3, max_length=12, eos=40, steps=5, seed=301, length_penalty=1.0, early_stopping=False)


def select_logprobs(rng, B, nb, V, eos):
    lp = (-rng.integers(0, 12, (B, nb, V)) * 0.5).astype(F32)
    lp[rng.random(lp.shape) < 0.3] = -np.inf
    top = rng.random((B, nb)) < 0.6
    lp[..., eos] = np.where(top, -0.5 * rng.integers(0, 2, (B, nb)), lp[..., eos]).astype(F32)
    lp[:, 0, : 2 * nb] = np.where(np.isfinite(lp[:, 0, : 2 * nb]), lp[:, 0, : 2 * nb], -5.5)
    return lp


@pytest.mark.parametrize("backend_name", ["torch", "ctypes"])
def test_beam_select_parents_chained_steps(backend_name):
    """Five chained steps from random candidates: everything kw_beam_select writes is bitwise what kw_beam_select
    writes on the same inputs, the parent log and the finished parents are the restatement's, and the backtrace of the
    best finished hypotheses is the oracle's ``beam_idx``."""
    from kwhisper.decode import beam_backtrace

    c = select_case()
    B, nb, V, P, ML, eos = c["B"], c["nb"], c["V"], c["P"], c["max_length"], c["eos"]
    rng = np.random.default_rng(c["seed"])
    prompt = np.array([[2, 4, 7], [2, 4, 9]])
    kw = dict(length_penalty=c["length_penalty"], early_stopping=c["early_stopping"])
    ref = T.BeamParentRef(prompt, nb, ML, eos=eos, fill=eos, **kw)
    plain = _State(prompt, nb, V, ML, eos, eos, **kw)
    par = _State(prompt, nb, V, ML, eos, eos, **kw)
    moved = False
    for step in range(c["steps"]):
        assert ref.go, f"the search ended before step {step}"
        lp = select_logprobs(rng, B, nb, V, eos)
        cv, ci = R.row_candidates(lp.reshape(B * nb, V), 2 * nb)
        for s in (plain, par):
            s.t["cand_val"].copy_(torch.from_numpy(cv))
            s.t["cand_idx"].copy_(torch.from_numpy(ci))
        plain.select(backend_name, False)
        par.select(backend_name, True)
        L0, old_par = ref.st["cur_len"], ref.fin_par.copy()
        info = ref.step(R.two_stage(lp, nb))
        moved |= any(src < nb and src != slot and old_par[b, src] != -1
                     for b in range(B) for slot, src in enumerate(info["fin_pick"][b]))
        torch.cuda.synchronize()
        for k in SEL_KEYS:
            a, b = plain.t[k], par.t[k]
            assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a,
                               b.view(torch.int32) if b.dtype == torch.float32 else b), (step, k)
        # and the shared state is the restatement's (so the comparison above is not of two idle launches)
        np.testing.assert_array_equal(par.t["ids"][:, : L0 + 1].cpu().numpy(),
                                      ref.st["running"].reshape(B * nb, -1)[:, : L0 + 1])
        np.testing.assert_array_equal(par.t["fin_flag"].cpu().numpy(), ref.st["fin"].astype(np.int32))
        np.testing.assert_array_equal(par.t["fin_len"].cpu().numpy(), ref.st["fin_len"])
        plog = par.t["parent_log"].cpu().numpy()
        np.testing.assert_array_equal(plog[P: L0 + 1], ref.plog[P: L0 + 1], err_msg=f"step {step}")
        assert (plog[:P] == -5).all() and (plog[L0 + 1:] == -5).all()  # one row per step, nothing else
        np.testing.assert_array_equal(par.t["fin_parent"].cpu().numpy(), ref.fin_par, err_msg=f"step {step}")
        assert (plain.t["parent_log"] == -5).all() and (plain.t["fin_parent"] == -1).all()
    st = ref.st
    assert st["fin"][:, 0].all() and ref.events["finish_in_top_nb"] > 0  # an EOS fired in every item
    assert any(len(set(ref.plog[P: P + c["steps"], r].tolist())) > 1 for r in range(B * nb))  # beams switched
    assert moved and set(ref.fin_par.reshape(-1).tolist()) - {-1, 0, nb}
    bi = beam_backtrace(par.t["parent_log"].cpu().numpy(), par.t["fin_parent"][:, 0].cpu().numpy(),
                        par.t["fin_len"][:, 0].cpu().numpy(), P)
    inside = np.arange(bi.shape[1]) < st["fin_len"][:, :1]
    np.testing.assert_array_equal(bi, np.where(inside, st["beam_idx"][:, 0, : bi.shape[1]], -1))


def test_beam_select_parents_rejects_bad_arguments():
    s = _State(np.array([[2, 4, 7]]), 3, 64, 12, 40, 40, 1.0, False)
    lib = L.load()
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    plog, fpar = ctypes.c_void_p(s.t["parent_log"].data_ptr()), ctypes.c_void_p(s.t["fin_parent"].data_ptr())
    before = {k: v.clone() for k, v in s.t.items()}
    assert lib.kw_beam_select_parents(ctypes.byref(s.b), None, fpar, stream) == L.KW_EINVAL
    assert lib.kw_beam_select_parents(ctypes.byref(s.b), plog, None, stream) == L.KW_EINVAL
    assert b"kw_beam_select_parents" in lib.kw_last_error()
    s.b.num_beams = 9
    assert lib.kw_beam_select_parents(ctypes.byref(s.b), plog, fpar, stream) == L.KW_EINVAL
    torch.cuda.synchronize()
    assert all(torch.equal(v, before[k]) for k, v in s.t.items())  # nothing was launched
