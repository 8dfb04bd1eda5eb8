"""The beam-search step kernels on the MI355X against the step-wise restatement (tests/_beam_ref.py over
oracle.generate.beam_step, the loop body that test_oracle_golden.py pins to transformers): kw_beam_logprobs,
kw_beam_select, the two in a closed loop on a toy model, and kw_self_attn_step with a slot table.

Indices, tokens, flags and everything kw_beam_select writes are compared exactly; log-prob values and attention
outputs within the tolerance each test states."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _beam_ref as R  # noqa: E402
from kwhisper import _lib as L  # noqa: E402
from kwhisper import ops  # noqa: E402

CANARY = -77
F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    L.load()
    torch.manual_seed(0)


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def cu(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda", dtype).contiguous()


class DevBeam:
    """The device state of a beam search, uploaded from a restatement state, and the two kernels' argument blocks.
    Rows are ``pad`` elements longer than max_length (ids, fin_seq, bp), the space beyond and every ids position
    the search has not reached hold a canary."""

    def __init__(self, st, bp, nb, V, max_length, P, *, eos, fill, length_penalty=1.0, early_stopping=False, gen=None,
                 rt=False, pad=(5, 3, 7), use_bp=True, split=False):
        B = st["running"].shape[0]
        Rn, K, L0 = B * nb, 2 * nb, st["cur_len"]
        self.B, self.nb, self.V, self.K, self.ML, self.use_bp = B, nb, V, K, max_length, use_bp
        ids = np.full((Rn, max_length + pad[0]), CANARY, np.int64)
        ids[:, :L0] = st["running"].reshape(Rn, -1)[:, :L0]
        fin_seq = np.full((B, nb, max_length + pad[1]), CANARY, np.int64)
        fin_seq[:, :, :max_length] = st["sequences"]
        bpa = np.full((Rn, max_length + pad[2]), CANARY, np.int32)
        bpa[:, :max_length] = bp
        self.exp = dict(ids=ids.copy(), fin_seq=fin_seq.copy(), bp=bpa.copy())
        i32 = torch.int32
        self.t = t = dict(
            ids=cu(ids, torch.int64), bp=cu(bpa, i32), run_scores=cu(st["run_scores"].reshape(-1), torch.float32),
            fin_seq=cu(fin_seq, torch.int64), fin_score=cu(st["beam_scores"], torch.float32),
            fin_len=cu(st["fin_len"], i32), fin_flag=cu(st["fin"].astype(np.int32), i32),
            unsat=cu(st["unsat"][:, 0].astype(np.int32), i32), cur_len=cu(np.array([L0]), i32),
            counter=torch.zeros(1, dtype=i32, device="cuda"), go=torch.zeros(1, dtype=i32, device="cuda"),
            done=torch.zeros(1, dtype=i32, device="cuda"), item_flags=torch.zeros((B, 3), dtype=i32, device="cuda"),
            cand_val=torch.zeros((Rn, K), device="cuda"), cand_idx=torch.zeros((Rn, K), dtype=i32, device="cuda"))
        b = self.b = L.BeamSelectArgs()
        b.B, b.num_beams, b.V = B, nb, V
        b.cand_val, b.cand_idx = t["cand_val"].data_ptr(), t["cand_idx"].data_ptr()
        b.ids, b.ids_stride = t["ids"].data_ptr(), t["ids"].stride(0)
        b.bp, b.bp_stride = (t["bp"].data_ptr(), t["bp"].stride(0)) if use_bp else (None, 0)
        b.run_scores = t["run_scores"].data_ptr()
        b.fin_seq, b.fin_stride = t["fin_seq"].data_ptr(), t["fin_seq"].shape[-1]
        b.fin_score, b.fin_len, b.fin_flag = t["fin_score"].data_ptr(), t["fin_len"].data_ptr(), t["fin_flag"].data_ptr()
        b.unsat, b.cur_len = t["unsat"].data_ptr(), t["cur_len"].data_ptr()
        b.begin_index, b.max_length, b.eos_id, b.fill_id = P, max_length, eos, fill
        b.length_penalty = float(length_penalty)
        b.early_stopping = 2 if early_stopping == "never" else int(bool(early_stopping))
        b.counter, b.go, b.done = t["counter"].data_ptr(), t["go"].data_ptr(), t["done"].data_ptr()
        b.item_flags = t["item_flags"].data_ptr()
        if gen is not None:
            t["logits"] = torch.zeros((Rn, V), device="cuda")
            sup = np.zeros(V, np.uint8)
            sup[gen["suppress_tokens"]] = 1
            t["sup"], t["bsup"] = cu(sup, torch.uint8), cu(np.array(gen["begin_suppress_tokens"]), i32)
            if split:
                t["ws"] = torch.zeros(ops.beam_logprobs_workspace_bytes(Rn) // 4 + 1, device="cuda")
            self.a = logprobs_args(t["logits"], t["sup"], t["bsup"], t["ids"], t["cur_len"], t["cand_val"],
                                   t["cand_idx"], t["done"], t.get("ws"), gen, rt, P, K)

    def logprobs(self):
        L.check(L.load().kw_beam_logprobs(ctypes.byref(self.a), _s()), "kw_beam_logprobs")

    def select(self):
        L.check(L.load().kw_beam_select(ctypes.byref(self.b), _s()), "kw_beam_select")

    def get(self):
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in self.t.items()}

    def check(self, ref, L_prev, what=""):
        """Every output of kw_beam_select against the restatement ``ref`` that has just made the same step."""
        got, st, e = self.get(), ref.st, self.exp
        e["ids"][:, :L_prev + 1] = st["running"].reshape(self.B * self.nb, -1)[:, :L_prev + 1]
        e["fin_seq"][:, :, :self.ML] = st["sequences"]
        if self.use_bp:
            e["bp"][:, :self.ML] = ref.bp
        want = dict(ids=e["ids"], bp=e["bp"], run_scores=st["run_scores"].reshape(-1), fin_seq=e["fin_seq"],
                    fin_score=st["beam_scores"], fin_len=st["fin_len"], fin_flag=st["fin"].astype(np.int32),
                    unsat=st["unsat"][:, 0].astype(np.int32), go=[int(ref.go)], done=[int(not ref.go)],
                    cur_len=[L_prev + 1], counter=[0])
        for k, w in want.items():
            np.testing.assert_array_equal(got[k], np.asarray(w), err_msg=f"{what} {k}")
        return got


def logprobs_args(logits, sup, bsup, ids, cur_len, cand_val, cand_idx, done, ws, gen, rt, P, k):
    a = L.BeamLogprobsArgs()
    a.logits, (a.R, a.V) = logits.data_ptr(), logits.shape
    a.suppress_mask, a.begin_suppress, a.n_begin_suppress = sup.data_ptr(), bsup.data_ptr(), bsup.numel()
    a.return_timestamps, a.ts_begin = int(rt), gen["no_timestamps_token_id"] + 1
    a.no_ts_id, a.eos_id = gen["no_timestamps_token_id"], gen["eos_token_id"]
    mit = gen.get("max_initial_timestamp_index")
    a.max_initial_ts = -1 if mit is None else mit
    a.ids, a.ids_stride, a.cur_len, a.begin_index, a.k = ids.data_ptr(), ids.stride(0), cur_len.data_ptr(), P, k
    a.cand_val, a.cand_idx, a.done = cand_val.data_ptr(), cand_idx.data_ptr(), done.data_ptr()
    a.workspace = ws.data_ptr() if ws is not None else None
    a.ws_bytes = ws.numel() * 4 if ws is not None else 0
    return a


# ---------------------------------------------------------------- (a) kw_beam_logprobs against the restatement
LP_RTOL, LP_ATOL = 1e-6, 1e-5
P0 = 3


def _lp_gen(V, k, layout):
    if layout == "spread":  # timestamps from token 10 on: their mass lies in all eight slices of the split kernel
        return {"suppress_tokens": [1], "begin_suppress_tokens": [3, 5], "eos_token_id": 5, "pad_token_id": 5,
                "no_timestamps_token_id": 9, "max_initial_timestamp_index": 50}
    if V < 50000:
        return R.toy_gen(V, k // 2)
    eos, ts_begin = 50257, V - 1501  # Whisper's layout: 1501 timestamps at the top
    rng = np.random.default_rng(V)
    sup = sorted(set(rng.integers(0, eos, 80).tolist()) | set(range(eos + 1, ts_begin - 1)))
    return {"suppress_tokens": sup, "begin_suppress_tokens": [220, eos], "eos_token_id": eos, "pad_token_id": eos,
            "no_timestamps_token_id": ts_begin - 1, "max_initial_timestamp_index": 50}


def _lp_inputs(Rn, V, k, kind):
    """Histories and logits for the processor states.  Row variants (by the last two tokens): 0 timestamp +
    timestamp, 1 text + timestamp, 2 timestamp + text, 3 text + text, 4 / 5 text + the last timestamp but one (three
    / two finite scores: fewer than k) with EOS above / below the timestamp mass.  Logits lie on a 0.5 grid with
    +-0.0 entries; k + 2 text tokens and k + 2 timestamps share the row's best value (a tie across the k-th
    place); even rows favour the timestamps (text banned by the mass rule), odd rows the text."""
    gen = _lp_gen(V, k, "real")
    rng = np.random.default_rng(Rn * 7 + V + k + len(kind))
    eos, ts = gen["eos_token_id"], gen["no_timestamps_token_id"] + 1
    variants = [4, 5, 0, 2] if Rn < 6 else [r % 6 for r in range(Rn)]
    n_hist = {"begin": 0, "pairs": 2, "long": 9}[kind]
    free = np.setdiff1d(np.arange(8, eos), gen["suppress_tokens"] + gen["begin_suppress_tokens"])
    hist = np.zeros((Rn, P0 + n_hist), np.int64)
    hist[:, :P0] = [2, 4, 7]
    x = (np.round(rng.standard_normal((Rn, V)) * 6) / 2).astype(F32)
    x[:, 5:40:3] = -0.0
    x[:, 6:40:3] = 0.0
    for r, var in enumerate(variants):
        if n_hist:
            text = rng.choice(free, 9)
            if n_hist == 9:  # earlier timestamps exist
                hist[r, P0:P0 + 7] = [ts + 1, ts + 1, text[0], text[1], ts + 3, ts + 3, text[2]]
            hist[r, -2:] = {0: [ts + 5, ts + 9], 1: [text[3], ts + 9], 2: [ts + 9, text[4]], 3: [text[5], text[6]],
                            4: [text[7], V - 2], 5: [text[8], V - 2]}[var]
        x[r, rng.choice(free, k + 2, replace=False)] = 20.0
        x[r, ts + 10 + rng.choice(40, k + 2, replace=False)] = 20.0 if r % 2 == 0 else 12.0
        if var in (4, 5):
            x[r, eos] = 25.0 if var == 4 else -5.0
            x[r, V - 2:] = 8.0
    return gen, hist, x


def _run_logprobs(gen, hist, x, k, rt, split, done=0, prefill=None):
    Rn, V = x.shape
    ids = torch.zeros((Rn, 64), dtype=torch.int64, device="cuda")
    ids[:, : hist.shape[1]] = cu(hist, torch.int64)
    cur = cu(np.array([hist.shape[1]]), torch.int32)
    sup = np.zeros(V, np.uint8)
    sup[gen["suppress_tokens"]] = 1
    keep = (cu(x, torch.float32), cu(sup, torch.uint8), cu(np.array(gen["begin_suppress_tokens"]), torch.int32), ids, cur,
            torch.full((Rn, k), 7.0 if prefill is None else prefill, device="cuda"),
            torch.full((Rn, k), 7 if prefill is None else int(prefill), dtype=torch.int32, device="cuda"),
            cu(np.array([done]), torch.int32),
            torch.zeros(ops.beam_logprobs_workspace_bytes(Rn) // 4 + 1, device="cuda") if split else None)
    a = logprobs_args(*keep, gen, rt, P0, k)
    for _ in range(2):  # the split kernel's arrival counters re-arm
        L.check(L.load().kw_beam_logprobs(ctypes.byref(a), _s()), "kw_beam_logprobs")
    torch.cuda.synchronize()
    return keep[5].cpu().numpy(), keep[6].cpu().numpy()


def _check_logprobs(gen, hist, x, k, rt, need_straddle=True):
    want = R.processed_logprobs(hist, x, gen, P0, rt)
    wv, wi = R.row_candidates(want, k)
    if rt:  # a condition on the inputs: the mass rule's decision is not a rounding question
        margin = R.timestamp_margin(hist, x, gen, P0)
        print("timestamp rule margins", np.round(margin, 4))
        assert (np.abs(margin) >= 1e-3).all(), margin
    if need_straddle:  # ... and some row's k-th and (k+1)-th best are equal
        srt = -np.sort(-want, axis=-1)
        assert (np.isfinite(srt[:, k]) & (srt[:, k - 1] == srt[:, k])).any()
    for split in (False, True):
        cv, ci = _run_logprobs(gen, hist, x, k, rt, split)
        fin = np.isfinite(wv) & np.isfinite(cv)
        err = np.abs(cv[fin] - wv[fin])
        print("split" if split else "one workgroup", "max |log-prob - reference|", err.max() if err.size else 0.0)
        np.testing.assert_array_equal(ci, wi, err_msg=f"split={split}")
        np.testing.assert_array_equal(np.isneginf(cv), np.isneginf(wv))
        np.testing.assert_allclose(cv, wv, rtol=LP_RTOL, atol=LP_ATOL, err_msg=f"split={split}")
    return wv, wi


@pytest.mark.parametrize("rt", [False, True])
@pytest.mark.parametrize("kind", ["begin", "pairs", "long"])
@pytest.mark.parametrize("Rn,V,k", [(4, 900, 16), (10, 51865, 10), (12, 51866, 4)])
def test_beam_logprobs_vs_reference(Rn, V, k, kind, rt):
    """Both kernels (one workgroup per row; a row split over eight) against process_logits(history,
    log_softmax(logits)) with the normaliser summed in float64.  Equal grid logits give bit-equal log-probs and
    unequal ones differ by >= 0.5, so the k candidate tokens must match exactly, order included -- also in the
    -inf places of a row with fewer than k finite scores (the lowest -inf tokens, as the reference's top-k names
    them and kw_beam_select keys them).  Values: the project's bound between its two f32 kernels (rtol 1e-6,
    atol 1e-5) is kept against float64.  For scale, torch.log_softmax in f32 (CPU) against float64 on these inputs
    is off by up to 7.5e-6 over a row and 6.8e-6 on the k candidates at V = 51865 / 51866 (its f32 normaliser),
    1.8e-6 / 2.3e-7 at V = 900; each run prints the kernels' own largest error."""
    gen, hist, x = _lp_inputs(Rn, V, k, kind)
    wv, _ = _check_logprobs(gen, hist, x, k, rt)
    if rt and kind != "begin" and Rn >= 6:  # rows 4, 5 (and 10, 11): three / two finite scores
        assert np.isneginf(wv[4, 3]) and np.isfinite(wv[4, 2]) and np.isneginf(wv[5, 2]) and np.isfinite(wv[5, 1])
    for split in (False, True):  # *done != 0: nothing is written
        cv, ci = _run_logprobs(gen, hist, x, k, rt, split, done=1, prefill=-3.0)
        assert (cv == -3.0).all() and (ci == -3).all()


@pytest.mark.parametrize("k", [10, 16])
def test_beam_logprobs_timestamp_mass_over_all_slices(k):
    """The mass rule where the split kernel's merge carries it: timestamps from token 10 on, all near 0.0, so that
    their log-sum-exp (10.86 = log 51856) comes from all eight slices in equal parts, against one text token at
    11.0 (even rows: text stays, margin -0.14) or 10.5 (odd rows: text banned, margin +0.36).  Under the ban the
    candidates are the lowest timestamps at the tied best value."""
    V, Rn = 51866, 4
    gen = _lp_gen(V, k, "spread")
    rng = np.random.default_rng(k)
    hist = np.array([[2, 4, 7, 6, 8]] * Rn, np.int64)
    x = np.zeros((Rn, V), F32)
    x[:, rng.choice(np.arange(10, V), 200, replace=False)] = -0.0
    x[:, :10] = (np.round(rng.standard_normal((Rn, 10)) * 4) / 2).clip(-6, 6)
    x[:, 0] = [11.0, 10.5, 11.0, 10.5]
    x[2:, rng.choice(np.arange(10, V), 100, replace=False)] = 0.5
    wv, wi = _check_logprobs(gen, hist, x, k, True, need_straddle=True)
    margin = R.timestamp_margin(hist, x, gen, P0)
    assert (margin[0::2] < 0).all() and (margin[1::2] > 0).all() and (np.abs(margin) < 0.5).all()
    assert (wi[1] >= 10).all() and wi[0, 0] == 0


# ---------------------------------------------------------------- (b) kw_beam_select, single hand-built steps
def _grid_logprobs(rng, B, nb, V, eos, sparsity):
    """Log-probs on a 0.5 grid (sums tie between beams, the same token in several), ``sparsity`` of them -inf, EOS
    near the top of about half the rows."""
    lp = (-rng.integers(0, 12, (B, nb, V)) * 0.5).astype(F32)
    lp[rng.random(lp.shape) < sparsity] = -np.inf
    top = rng.random((B, nb)) < 0.5
    lp[..., eos] = np.where(top, -0.5 * rng.integers(0, 3, (B, nb)), lp[..., eos]).astype(F32)
    return lp


def _select_step(st, bp, lp, nb, P, max_length, eos, fill, *, length_penalty=1.0, early_stopping=False, use_bp=True,
                 cands_from=None):
    """One kw_beam_select launch on the candidates the CPU takes from ``lp`` (B, nb, V); every output against
    beam_step's flat top-k over the whole of ``lp``."""
    B, _, V = lp.shape
    kw = dict(eos=eos, fill=fill, length_penalty=length_penalty, early_stopping=early_stopping)
    ref = R.BeamRef.from_state(st, bp, nb, max_length, P, **kw)
    dev = DevBeam(st, bp, nb, V, max_length, P, use_bp=use_bp, **kw)
    cv, ci = R.row_candidates((lp if cands_from is None else cands_from).reshape(B * nb, V), 2 * nb)
    dev.t["cand_val"].copy_(cu(cv, torch.float32))
    dev.t["cand_idx"].copy_(cu(ci, torch.int32))
    dev.select()
    L0 = st["cur_len"]
    info = ref.step(lp)
    dev.check(ref, L0)
    return ref, info, dev


SELECT_SHAPES = ([(3, 5, 64, es, lpn, True) for es in (False, True, "never") for lpn in (0.0, 0.5, 1.0, 2.0, -0.5)] +
                 [(1, 2, 64, False, 1.0, True), (3, 8, 64, True, 1.0, True), (70, 8, 64, False, 1.0, True),
                  (70, 2, 64, True, 0.5, True), (2, 8, 51866, False, 1.0, True), (1, 5, 51866, "never", 2.0, True),
                  (3, 5, 64, True, 1.0, False), (70, 8, 64, False, 2.0, False)])


@pytest.mark.parametrize("B,nb,V,es,lpn,use_bp", SELECT_SHAPES)
def test_beam_select_random_steps(B, nb, V, es, lpn, use_bp):
    """Random mid-search states (tests/_beam_ref.py::mid_state): grid scores and grid log-probs (ties between beams
    and inside the merge), dense and mostly suppressed rows, finished sets from empty to full, items that have
    stopped improving beside ones that have not, dead (-1e9) rows, all running scores equal (the flat index
    decides, up to beam 7 x 51866), the step that reaches max_length, strides longer than max_length with a canary
    beyond, with and without a slot table."""
    rng = np.random.default_rng(B * 1000 + nb * 10 + V)
    P, eos = 3, V * 5 // 8
    seen = R.collections.Counter()
    for trial in range(6):
        L0 = int(rng.integers(P, P + 6))
        max_length = L0 + 1 if trial == 4 else L0 + 4
        unsat = rng.random(B) < 0.7
        if B > 1:
            unsat[:2] = [False, True]
        st, bp = R.mid_state(rng, B, nb, V, P, L0, max_length, eos, n_dead=trial % 2, unsat=unsat,
                             n_fin=nb if trial == 3 else None)
        if trial == 5:
            st["run_scores"][:] = -1.5
        lp = _grid_logprobs(rng, B, nb, V, eos, 0.9 if trial == 2 else 0.3)
        if trial % 2:  # the live rows fill the top 2 nb (include/kwhisper.h)
            lp[:, 0, : 2 * nb] = np.where(np.isfinite(lp[:, 0, : 2 * nb]), lp[:, 0, : 2 * nb], -5.5)
        ref, info, _ = _select_step(st, bp, lp, nb, P, max_length, eos, eos, length_penalty=lpn, early_stopping=es,
                                    use_bp=use_bp)
        seen.update(ref.events)
        seen["eos_below_top_nb"] += int((info["tok"][:, nb:] == eos).any())
        seen["last_parent"] += int((info["parent"] == nb - 1).any())
    print(dict(seen))
    if B >= 3:  # (with fewer items six steps need not hold every event)
        for k in ("finish_in_top_nb", "tie_among_kept", "eos_below_top_nb", "last_parent"):
            assert seen[k] > 0, (k, dict(seen))


def _bare_state(B, nb, V, P, L0, max_length, fill, seed=0):
    rng = np.random.default_rng(seed)
    return R.mid_state(rng, B, nb, V, P, L0, max_length, fill, n_fin=0)


def test_beam_select_merge_tie_keeps_the_old_entry_first():
    """A new finished sequence whose penalised score equals an old one's: the old entry has the lower key."""
    nb, V, P, L0, eos = 2, 64, 3, 6, 40
    st, bp = _bare_state(1, nb, V, P, L0, 10, eos)
    st["run_scores"][:] = [[0.0, -0.5]]
    st["fin"][0, 0], st["beam_scores"][0, 0], st["fin_len"][0, 0] = True, -1.0, 2
    st["sequences"][0, 0, P:P + 2] = [9, eos]
    lp = np.full((1, nb, V), -6.0, F32)
    lp[0, 0, eos] = -4.0  # rank 0: -4.0 / (L0 + 1 - P) ** 1.0 = -1.0
    ref, info, _ = _select_step(st, bp, lp, nb, P, 10, eos, eos)
    assert info["tok"][0, 0] == eos and ref.st["beam_scores"].tolist() == [[-1.0, -1.0]]
    assert ref.st["fin_len"].tolist() == [[2, 4]] and ref.st["fin"].all()


def test_beam_select_signed_zero_sums_tie():
    """-0.0 (beam 0) and +0.0 (beam 1) are one value: the lower flat index goes first, not the larger bit pattern."""
    nb, V, P, L0, eos = 2, 64, 3, 5, 40
    st, bp = _bare_state(1, nb, V, P, L0, 10, eos)
    st["run_scores"][:] = [[-0.0, 0.0]]
    lp = np.full((1, nb, V), -3.0, F32)
    lp[0, 0, 5] = lp[0, 1, 3] = -0.0
    ref, info, _ = _select_step(st, bp, lp, nb, P, 10, eos, eos)
    assert info["parent"][0, :2].tolist() == [0, 1] and info["tok"][0, :2].tolist() == [5, 3]
    assert np.signbit(info["topk_lp"][0, 0]) and not np.signbit(info["topk_lp"][0, 1])


def test_beam_select_eos_below_the_top_nb_does_not_finish():
    nb, V, P, L0, eos = 2, 64, 3, 5, 40
    st, bp = _bare_state(1, nb, V, P, L0, 10, eos)
    st["run_scores"][:] = [[0.0, -1.0]]
    lp = np.full((1, nb, V), -9.0, F32)
    lp[0, 0, [11, 12, eos, 13]] = [-1.0, -2.0, -3.0, -4.0]  # EOS at rank 2 = nb
    ref, info, _ = _select_step(st, bp, lp, nb, P, 10, eos, eos)
    assert info["tok"][0].tolist() == [11, 12, eos, 13] and not ref.st["fin"].any() and ref.go


def test_beam_select_full_finished_set_better_and_worse():
    """Both items hold nb finished sequences; item 0's new one beats them all and displaces the worst, item 1's is
    worse than all and leaves the set alone (length_penalty 0: the score is the sum itself)."""
    nb, V, P, L0, eos = 5, 64, 3, 6, 40
    rng = np.random.default_rng(5)
    st, bp = R.mid_state(rng, 2, nb, V, P, L0, 12, eos, n_fin=nb)
    st["run_scores"][:, 0] = 0.0
    lp = np.full((2, nb, V), -9.0, F32)
    lp[:, :, 20:30] = -8.0
    lp[0, 0, eos], lp[1, 0, eos] = -0.25, -4.0
    before = st["beam_scores"].copy()
    ref, info, _ = _select_step(st, bp, lp, nb, P, 12, eos, eos, length_penalty=0.0)
    assert (info["tok"][:, 0] == eos).all()
    assert ref.st["beam_scores"][0, 0] == -0.25 and ref.st["beam_scores"][0, 1:].tolist() == before[0, :-1].tolist()
    assert ref.st["beam_scores"][1].tolist() == before[1].tolist()


def test_beam_select_all_hit_at_max_length():
    """The step with L + 1 == max_length: every continuation hits MaxLength, the top nb finish whatever their
    token, and the search stops on all_hit.  (2 nb EOS continuations of one item cannot occur otherwise: a beam
    holds the EOS token once, and an item has nb beams.)"""
    nb, V, P, L0, eos = 5, 64, 3, 7, 40
    rng = np.random.default_rng(9)
    st, bp = R.mid_state(rng, 3, nb, V, P, L0, L0 + 1, eos, n_fin=0)
    lp = _grid_logprobs(rng, 3, nb, V, eos, 0.3)
    ref, info, _ = _select_step(st, bp, lp, nb, P, L0 + 1, eos, eos)
    assert info["hits"].all() and not ref.go and ref.st["fin"].all() and ref.events["stop_all_hit"] == 1


def test_beam_select_histories_to_the_lds_bound():
    """max_length 512 from begin_index 506: six steps take the histories, the slot tables and the finished rows to
    the 512 entries the kernel's LDS arrays hold; nb 8, two items, every step compared."""
    nb, V, P, ML, eos, B = 8, 64, 506, 512, 40, 2
    rng = np.random.default_rng(512)
    prompt = rng.integers(0, V, (B, P))
    kw = dict(eos=eos, fill=eos, length_penalty=1.0, early_stopping=False)
    ref = R.BeamRef(prompt, nb, ML, **kw)
    dev = DevBeam(ref.st, ref.bp, nb, V, ML, P, **kw)
    steps = 0
    while ref.go:
        lp = _grid_logprobs(rng, B, nb, V, eos, 0.3)
        lp[..., eos] -= 3.0  # (keep the search going to the last position)
        cv, ci = R.row_candidates(lp.reshape(B * nb, V), 2 * nb)
        dev.t["cand_val"].copy_(cu(cv, torch.float32))
        dev.t["cand_idx"].copy_(cu(ci, torch.int32))
        dev.select()
        L0 = ref.st["cur_len"]
        ref.step(lp)
        dev.check(ref, L0, f"step {steps}")
        steps += 1
    assert steps == 6 and ref.st["cur_len"] == 512


def test_beam_select_pins_the_documented_exception():
    """include/kwhisper.h: where the top 2 nb reaches into a -1e9 row, the kernel keeps the lowest ids among that
    row's 2 nb best log-probs (the restatement's two_stage), the reference its lowest ids overall."""
    nb, V, P, L0, eos = 2, 64, 3, 5, 7
    st, bp = _bare_state(1, nb, V, P, L0, 10, 63)
    st["run_scores"][:] = [[-3.0, R.NEG]]
    lp = np.full((1, nb, V), -np.inf, F32)
    lp[0, 0, [10, 11]] = [-0.5, -1.0]
    lp[0, 1, :] = -20.0
    lp[0, 1, [40, 41, 42, 43]] = [-1.0, -2.0, -3.0, -4.0]
    kw = dict(eos=eos, fill=63)
    ref = R.BeamRef.from_state(st, bp, nb, 10, P, **kw)
    dev = DevBeam(st, bp, nb, V, 10, P, **kw)
    cv, ci = R.row_candidates(lp.reshape(nb, V), 2 * nb)
    dev.t["cand_val"].copy_(cu(cv, torch.float32))
    dev.t["cand_idx"].copy_(cu(ci, torch.int32))
    dev.select()
    info = ref.step(R.two_stage(lp, nb))
    dev.check(ref, L0)
    assert info["tok"].tolist() == [[10, 11, 40, 41]]


def test_beam_select_rejects_bad_arguments():
    nb, V, P, L0, eos = 2, 64, 3, 5, 40
    st, bp = _bare_state(1, nb, V, P, L0, 10, eos)
    dev = DevBeam(st, bp, nb, V, 10, P, eos=eos, fill=eos)
    lib, b = L.load(), dev.b

    def rc(**kw):
        old = {k: getattr(b, k) for k in kw}
        for k, v in kw.items():
            setattr(b, k, v)
        out = lib.kw_beam_select(ctypes.byref(b), _s())
        for k, v in old.items():
            setattr(b, k, v)
        return out

    assert rc(num_beams=1) == L.KW_EINVAL and rc(num_beams=9) == L.KW_EINVAL
    assert rc(max_length=513, ids_stride=600, fin_stride=600, bp_stride=600) == L.KW_EINVAL
    assert rc(fin_stride=9) == L.KW_EINVAL and rc(bp_stride=9) == L.KW_EINVAL and rc(ids_stride=9) == L.KW_EINVAL
    got = dev.get()
    assert got["cur_len"][0] == L0 and got["counter"][0] == 0  # nothing ran


# ---------------------------------------------------------------- (c) the two kernels in a closed loop
def _case_id(c):
    return "V{}-nb{}-ts{}-es{}-lp{}-s{}-n{}".format(*[int(v) if isinstance(v, bool) else v for v in c])


@pytest.mark.parametrize("case", R.CLOSED_LOOP_CASES, ids=_case_id)
def test_beam_closed_loop_on_the_toy_model(case):
    """The toy model (logits = table[last token], evaluated on the device by an index select) under both kernels
    until go == 0.  Per step: kw_beam_logprobs against the reference on the device's own histories (as in (a)),
    then kw_beam_select's whole state against beam_step applied to the device's candidates, scattered into a -inf
    array -- the comparison follows the device, so a last-ulp difference in a log-prob cannot fork it -- and the
    slot-table invariant against a shadow of what each (cache row, position) was fed.  Then two more launches of
    both kernels: nothing changes (the graph-replay contract).  Odd seeds use the split log-probs kernel.
    tests/test_beam_cpu.py::test_closed_loop_cases_cover_the_events asserts that these cases hold, between them, a
    finish inside the top nb, an exact tie among the kept sums, a displaced finished entry, an item that stops
    improving beside one that goes on, a stop through each clause of go, and a row short of finite candidates."""
    V, nb, rt, es, lpn, seed, _ = case
    gen, table, ML, kw = R.case_setup(case)
    prompt, K = R.CLOSED_LOOP_PROMPT, 2 * nb
    B, P = prompt.shape
    Rn = B * nb
    kw.update(eos=gen["eos_token_id"], fill=gen["pad_token_id"])
    ref = R.BeamRef(prompt, nb, ML, **kw)
    dev = DevBeam(ref.st, ref.bp, nb, V, ML, P, gen=gen, rt=rt, split=bool(seed % 2), **kw)
    tab = cu(table, torch.float32)
    shadow = np.full((Rn, ML), -1, np.int64)
    shadow[:, :P] = np.repeat(prompt, nb, 0)
    while ref.go:
        L0 = ref.st["cur_len"]
        hist = ref.history()  # == the device's ids[:, :L0] (checked after the last step)
        dev.t["logits"].copy_(tab.index_select(0, dev.t["ids"][:, L0 - 1]))
        dev.logprobs()
        torch.cuda.synchronize()
        cv, ci = dev.t["cand_val"].cpu().numpy(), dev.t["cand_idx"].cpu().numpy()
        if rt:
            # a condition on the inputs.  (Exactly 0: one timestamp left, its grid logit equal to the best text
            # token's -- the same number on both sides in any arithmetic, and the rule's > does not fire.)
            margin = R.timestamp_margin(hist, table[hist[:, -1]], gen, P)
            assert ((np.abs(margin) >= 1e-3) | (margin == 0)).all(), margin
        wv, wi = R.row_candidates(R.processed_logprobs(hist, table[hist[:, -1]], gen, P, rt), K)
        np.testing.assert_array_equal(ci, wi, err_msg=f"L={L0}")
        np.testing.assert_allclose(cv, wv, rtol=LP_RTOL, atol=LP_ATOL, err_msg=f"L={L0}")
        dev.select()
        ref.step(R.scatter_candidates(cv.reshape(B, nb, K), ci.reshape(B, nb, K), V))
        got = dev.check(ref, L0, f"L={L0}")
        shadow[:, L0] = got["ids"][:, L0]  # what row r is fed at position L0 next step lands in cache row r
        cols = np.arange(L0 + 1)
        for r in range(Rn):
            np.testing.assert_array_equal(shadow[got["bp"][r, : L0 + 1], cols], got["ids"][r, : L0 + 1])
    before = {k: v.clone() for k, v in dev.t.items()}
    for _ in range(2):
        dev.logprobs()
        dev.select()
    torch.cuda.synchronize()
    for k, v in before.items():
        assert torch.equal(v.view(torch.uint8) if v.is_floating_point() else v,
                           dev.t[k].view(torch.uint8) if v.is_floating_point() else dev.t[k]), k


# ---------------------------------------------------------------- (d) kw_self_attn_step with a slot table
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("past", [1, 10, 255, 256, 300, 447])
def test_self_attn_step_slot_table(dtype, past):
    """Six rows (two items x three beams) whose key/value position k < L - 1 lives in cache row bp[r][k]: a
    different permutation of the item's rows at every position, the row itself at L - 1, and beyond L another
    valid row (a kernel that read it would show a wrong number).  Every cache row holds distinct data.  Reference:
    the gather, softmax and weighted sum in float64; tolerances are test_self_attn_step's.  The launch writes
    [r][h][L - 1] of the caches and nothing else, a second launch gives the same bits (the arrival counters re-arm),
    and the identity table is the bp=None call bit for bit."""
    B, H, hd, t_max, nbm = 6, 2, 64, 448, 3
    d, Lc = H * hd, past + 1
    g = torch.Generator().manual_seed(past)
    kc0 = torch.randn(B, H, t_max, hd, generator=g).to("cuda", dtype)
    vc0 = torch.randn(B, H, t_max, hd, generator=g).to("cuda", dtype)
    qkv = torch.randn(B, 3 * d, generator=g).to("cuda", dtype)
    rng = np.random.default_rng(past)
    bp = np.empty((B, t_max + 8), np.int32)
    bp[:] = ((np.arange(B) + 1) % nbm + np.arange(B) // nbm * nbm)[:, None]  # beyond L: another row of the item
    for k in range(past):
        for item in range(B // nbm):
            bp[item * nbm:(item + 1) * nbm, k] = item * nbm + rng.permutation(nbm)
    bp[:, past] = np.arange(B)
    bpt = cu(bp, torch.int32)
    cur = cu(np.array([Lc]), torch.int32)
    ws = torch.zeros(ops.self_attn_workspace_bytes(B, H, t_max) // 4 + 1, device="cuda")

    def run(table):
        kc, vc = kc0.clone(), vc0.clone()
        out = torch.full((B, d), float("nan"), device="cuda").to(dtype)
        ops.self_attn_step(qkv, B, 1, H, hd, kc, vc, t_max, cur, out, ws, bp=table)
        first = out.clone()
        ops.self_attn_step(qkv, B, 1, H, hd, kc, vc, t_max, cur, out, ws, bp=table)
        torch.cuda.synchronize()
        assert torch.equal(first.view(torch.uint8), out.view(torch.uint8))
        return out, kc, vc

    out, kc, vc = run(bpt)
    x = qkv.double().view(B, 3, H, hd)
    rows = torch.from_numpy(bp[:, :past].astype(np.int64)).cuda()  # (B, past)
    pos = torch.arange(past, device="cuda")
    k_all = torch.cat([kc0.double()[rows, :, pos].permute(0, 2, 1, 3), x[:, 1].unsqueeze(2)], 2)  # (B, H, L, hd)
    v_all = torch.cat([vc0.double()[rows, :, pos].permute(0, 2, 1, 3), x[:, 2].unsqueeze(2)], 2)
    s = (x[:, 0].unsqueeze(2) @ k_all.transpose(-1, -2))
    ref = (torch.softmax(s, -1) @ v_all).reshape(B, d).float()
    tol = 1e-5 if dtype == torch.float32 else 2e-2
    torch.testing.assert_close(out.float(), ref, atol=tol, rtol=tol)
    want_k, want_v = kc0.clone(), vc0.clone()
    want_k[:, :, past] = qkv.view(B, 3, H, hd)[:, 1]
    want_v[:, :, past] = qkv.view(B, 3, H, hd)[:, 2]
    assert torch.equal(kc.view(torch.uint8), want_k.view(torch.uint8))
    assert torch.equal(vc.view(torch.uint8), want_v.view(torch.uint8))
    ident = cu(np.tile(np.arange(B, dtype=np.int32)[:, None], (1, t_max)), torch.int32)
    o_id, _, _ = run(ident)
    o_none, _, _ = run(None)
    assert torch.equal(o_id.view(torch.uint8), o_none.view(torch.uint8))
    if past == 10:  # a table with q_len = 2 is refused
        dt = L.KW_DT_F32 if dtype == torch.float32 else L.KW_DT_BF16
        q2 = torch.zeros(B * 2, 3 * d, device="cuda", dtype=dtype)
        o2 = torch.zeros(B * 2, d, device="cuda", dtype=dtype)
        vp = ctypes.c_void_p
        rc = L.load().kw_self_attn_step(dt, vp(q2.data_ptr()), B, 2, H, hd, vp(kc.data_ptr()), vp(vc.data_ptr()), t_max,
                                        vp(cur.data_ptr()), vp(bpt.data_ptr()), bpt.stride(0), vp(o2.data_ptr()),
                                        vp(ws.data_ptr()), ws.numel() * 4, _s())
        assert rc == L.KW_EINVAL
