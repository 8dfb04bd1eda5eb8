"""The step-wise beam-search restatement (oracle.generate.beam_step, tests/_beam_ref.py) on the CPU: it reproduces
the loop it was factored out of, and the design claim of csrc/beam.hip -- per-row candidates, then the flat
top-k over the candidates -- is checked against the reference's flat top-k over beams x vocab."""
import itertools

import numpy as np
import pytest

import _beam_ref as R
from oracle import generate as og

PROMPT = np.array([[2, 4, 7], [2, 4, 9], [2, 4, 12]])

# beam_search(ToyModel(grid_table(V, seed, eos_boost=(seed % 3) * 1.5, ts_boost=rt)), ...) of the commit before
# beam_step was factored out (its oracle/generate.py loaded beside this one), max_length 15:
# (V, nb, return_timestamps, early_stopping, length_penalty, seed) -> tokens
FROZEN = {
    (64, 2, False, False, 1.0, 0): [[2, 4, 7, 33, 53, 29, 53, 29, 53, 29, 53, 29, 53, 29, 53],
                                    [2, 4, 9, 27, 36, 13, 16, 27, 36, 35, 3, 27, 36, 35, 3],
                                    [2, 4, 12, 11, 53, 29, 53, 29, 53, 29, 53, 29, 53, 29, 53]],
    (64, 5, True, True, 0.5, 1): [[2, 4, 7, 53, 40, 40, 40, 40], [2, 4, 9, 52, 35, 53, 54, 40],
                                  [2, 4, 12, 56, 40, 40, 40, 40]],
    (200, 8, True, "never", 2.0, 2): [[2, 4, 7, 170, 112, 182, 189, 2, 72, 80, 191, 192, 56, 0, 195],
                                      [2, 4, 9, 150, 4, 164, 178, 0, 195, 196, 112, 0, 56, 0, 56],
                                      [2, 4, 12, 150, 4, 164, 178, 0, 179, 189, 2, 72, 80, 191, 192]],
    (200, 5, False, True, -0.5, 4): [[2, 4, 7, 183, 72, 65, 162, 31, 23, 125], [2, 4, 9, 185, 30, 77, 125, 125, 125, 125],
                                     [2, 4, 12, 69, 27, 100, 125, 125, 125, 125]],
}


def _toy(V, nb, rt, seed):
    gen = R.toy_gen(V, nb, mostly_suppressed=(seed % 3 == 2))
    return gen, R.grid_table(V, seed, eos_boost=(seed % 3) * 1.5, ts_boost=1.0 if rt else 0.0)


@pytest.mark.parametrize("case", sorted(FROZEN, key=str), ids=str)
def test_factored_step_reproduces_the_loop(case):
    V, nb, rt, es, lpn, seed = case
    gen, table = _toy(V, nb, rt, seed)
    got = og.beam_search(R.ToyModel(table), np.zeros((3, 1)), PROMPT, gen, 15, 3, rt, nb, lpn, es)
    np.testing.assert_array_equal(got, np.asarray(FROZEN[case]))
    # and the step-wise driver of the GPU tests walks the same search
    ref, _ = R.closed_loop(table, PROMPT, nb, 15, gen, rt, length_penalty=lpn, early_stopping=es)
    n = got.shape[1]
    best = ref.st["sequences"][:, 0]
    np.testing.assert_array_equal(best[:, :n], got)
    assert (best[:, n:] == gen["pad_token_id"]).all() and int(ref.st["fin_len"][:, 0].max()) == n - 3


# ---- two-stage selection == flat top-k -----------------------------------------------------------------------------
@pytest.mark.parametrize("V,nb", [(64, 2), (64, 5), (64, 8), (200, 2), (200, 5), (200, 8)])
def test_two_stage_selection_is_the_flat_topk_closed_loop(V, nb):
    """Markov tables on a 0.5 grid (exact ties), three items, 12 new tokens, timestamps on and off, the three
    early_stopping modes, five length penalties, a mostly suppressed vocabulary every third seed: the search that
    sees only each row's 2 nb candidates goes through the same states as the one that sees the whole rows."""
    ev = R.collections.Counter()
    for rt, es, seed in itertools.product((False, True), (False, True, "never"), range(6)):
        gen, table = _toy(V, nb, rt, seed)
        kw = dict(length_penalty=(1.0, 0.5, 2.0, 0.0, -0.5, 1.0)[seed], early_stopping=es)
        a, ta = R.closed_loop(table, PROMPT, nb, 15, gen, rt, **kw)
        b, tb = R.closed_loop(table, PROMPT, nb, 15, gen, rt, selection=R.two_stage, **kw)
        assert len(ta) == len(tb) and all(R.same_state(x, y) for x, y in zip(ta, tb)), (rt, es, seed)
        np.testing.assert_array_equal(a.bp, b.bp)
        ev.update(a.events)
    # the cases are not vacuous
    for k in ("finish_in_top_nb", "tie_among_kept", "row_short_of_candidates", "finished_displaced"):
        assert ev[k] > 0, (k, dict(ev))


def _one_step_state(rng, B, nb, V, L, P, n_dead):
    """A mid-search state: distinct histories, scores on a grid (ties between beams), ``n_dead`` trailing rows per
    item at -1e9."""
    st = og.beam_init(rng.integers(0, 8, (B, P)), nb, L + 4, fill=V - 1)
    st["running"][:, :, P:L] = rng.integers(0, V, (B, nb, L - P))
    st["cur_len"] = L
    sc = -np.sort(rng.integers(0, 6, (B, nb)) * 0.5, axis=1).astype(np.float32)
    if n_dead:
        sc[:, nb - n_dead:] = R.NEG
    st["run_scores"] = -np.sort(-sc, axis=1)
    return st


@pytest.mark.parametrize("nb", [2, 5, 8])
@pytest.mark.parametrize("n_dead", [0, 1])
def test_two_stage_selection_single_steps(nb, n_dead):
    """Hand-built steps: log-probs on a 0.5 grid, rows with fewer than 2 nb finite scores (down to none), most of
    the vocabulary suppressed, rows at -1e9 -- as long as the live rows fill the top 2 nb (the documented
    condition; see test_two_stage_selection_differs_where_a_score_absorbs_the_logprobs)."""
    rng = np.random.default_rng(nb * 10 + n_dead)
    V, B, P, L = 64, 4, 2, 5
    for trial in range(40):
        st = _one_step_state(rng, B, nb, V, L, P, n_dead)
        lp = (-rng.integers(0, 12, (B, nb, V)) * 0.5).astype(np.float32)
        lp[rng.random((B, nb, V)) < (0.9 if trial % 2 else 0.3)] = -np.inf  # mostly suppressed / dense
        for b in range(B):
            j = rng.integers(0, nb)
            keep = rng.integers(0, 2 * nb)  # a row short of candidates: `keep` finite scores (0 = none)
            fin = np.flatnonzero(np.isfinite(lp[b, j]))
            lp[b, j, fin[keep:]] = -np.inf
        live = nb - n_dead
        if n_dead:  # the live rows of each item hold the 2 nb best
            short = np.isfinite(lp[:, :live]).sum((1, 2)) < 2 * nb
            lp[short, 0, : 2 * nb] = -1.0
        kw = dict(eos=7, max_length=L + 4, begin_index=P, length_penalty=1.0, early_stopping=False)
        a, ia = og.beam_step(lp, st, **kw)
        b2, ib = og.beam_step(R.two_stage(lp, nb), st, **kw)
        assert R.same_state(a, b2) and ia["go"] == ib["go"], trial
        np.testing.assert_array_equal(ia["hits"], ib["hits"])


def test_two_stage_selection_differs_where_a_score_absorbs_the_logprobs():
    """The exception stated in include/kwhisper.h, pinned: the live row holds fewer than 2 nb finite candidates,
    so the top 2 nb reaches into a row at -1e9, where every log-prob above -32 rounds to the same f32 sum.  The
    reference's flat top-k then takes that row's lowest token ids; the two-stage selection takes the lowest ids
    among the row's 2 nb best log-probs."""
    nb, V, P, L = 2, 64, 2, 4
    st = og.beam_init(np.array([[1, 2]]), nb, 8, fill=63)
    st["cur_len"] = L
    st["run_scores"] = np.array([[-3.0, R.NEG]], np.float32)
    lp = np.full((1, nb, V), -np.inf, np.float32)
    lp[0, 0, [10, 11]] = [-0.5, -1.0]               # the live row: two candidates, four places
    lp[0, 1, :] = -20.0
    lp[0, 1, [40, 41, 42, 43]] = [-1.0, -2.0, -3.0, -4.0]  # the dead row's best sit at high ids
    assert np.float32(-20.0) + R.NEG == np.float32(-1.0) + R.NEG == R.NEG
    kw = dict(eos=7, max_length=8, begin_index=P)
    flat, fi = og.beam_step(lp, st, **kw)
    two, ti = og.beam_step(R.two_stage(lp, nb), st, **kw)
    np.testing.assert_array_equal(fi["tok"], [[10, 11, 0, 1]])
    np.testing.assert_array_equal(ti["tok"], [[10, 11, 40, 41]])
    np.testing.assert_array_equal(fi["topk_lp"], ti["topk_lp"])  # the same sums: only the tie is split differently
    np.testing.assert_array_equal(flat["running"][0, :, L], two["running"][0, :, L])  # the running rows agree here


# ---- the slot table and the committed closed-loop cases ------------------------------------------------------------
def test_slot_table_names_the_row_that_was_fed_each_position():
    """BeamRef.bp against its definition: feed every running row's last token into "its" cache row each step;
    bp[r][p] then names a row whose position p holds the token ids[r][p]."""
    gen, table = _toy(64, 5, True, 3)
    ref = R.BeamRef(PROMPT, 5, 15, eos=gen["eos_token_id"], fill=gen["pad_token_id"])
    shadow = np.full((15, 15), -1, np.int64)
    shadow[:, :3] = np.repeat(PROMPT, 5, 0)
    moved = 0
    while ref.go:
        hist = ref.history()
        lp = R.processed_logprobs(hist, table[hist[:, -1]], gen, 3, True)
        ref.step(lp)
        L = ref.st["cur_len"]
        ids = ref.st["running"].reshape(15, -1)
        shadow[:, L - 1] = ids[:, L - 1]
        for r in range(15):
            np.testing.assert_array_equal(shadow[ref.bp[r, :L], np.arange(L)], ids[r, :L])
        moved += int((ref.bp[:, :L] != np.arange(15)[:, None]).any())
    assert moved > 0


def test_closed_loop_cases_cover_the_events():
    """The cases tests/test_gpu_beam_kernels.py runs on the device, walked here on the CPU: between them they hold
    every event the kernels branch on."""
    ev = R.collections.Counter()
    for case in R.CLOSED_LOOP_CASES:
        ref, _ = R.run_case(case)
        ev.update(ref.events)
    print(dict(ev))
    for k in ("finish_in_top_nb", "tie_among_kept", "finished_displaced", "item_stops_improving_alone",
              "stop_no_improve_alone", "stop_all_fin_alone", "stop_all_hit", "row_short_of_candidates"):
        assert ev[k] > 0, (k, dict(ev))
