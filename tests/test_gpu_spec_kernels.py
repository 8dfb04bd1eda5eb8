"""GPU tests of kw_spec_accept (csrc/spec.hip): one launch against K + 1 sequential kw_greedy_step launches on the same
random logits and histories (the drafts in place) followed by the accept walk of tests/_spec_ref.py -- ids, lengths,
flags and counters equal, the per-position tokens also equal to the pinned processors' arg-max
(oracle.generate.process_logits) -- through both backends, over the draft patterns a round can meet."""
import numpy as np
import pytest
import torch

import _spec_ref as R
from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs the MI355X")]

P = 3
PATTERNS = ["none", "all", "upto", "eos_accepted", "eos_correction", "maxlen", "first", "pair", "mass"]


def _gen(V):
    """Generation constants (a dict, as oracle.generate takes them) for vocabulary size V; V = 1000 has its own small
    layout: text [0, 880), EOS 880, specials, <|notimestamps|> 899, timestamps [900, 1000)."""
    from kwhisper.config import LARGE_V3, TINY, generation_constants

    if V == 1000:
        return dict(eos_token_id=880, pad_token_id=879, no_timestamps_token_id=899, max_initial_timestamp_index=50,
                    suppress_tokens=[1, 2, 7, 300, 511, 512] + list(range(881, 899)), begin_suppress_tokens=[220, 880])
    return generation_constants({51865: TINY, 51866: LARGE_V3, 65545: LARGE_V3}[V]).to_dict()


def _scenario(V, K, rt, pattern, rng):
    """(history, drafts, logits [K + 1][V], max_length) of one pattern; the drafts are built from the pinned
    processors' tokens so that exactly the intended prefix agrees."""
    gd = _gen(V)
    eos, tsb = gd["eos_token_id"], gd["no_timestamps_token_id"] + 1
    ok = np.setdiff1d(np.arange(3, eos - 1), np.asarray(gd["suppress_tokens"] + gd["begin_suppress_tokens"]))
    prompt = [tsb - 107, tsb - 99, tsb - 6] if tsb > 1000 else [890, 891, 892]
    body = [] if pattern == "first" else [tsb + 2] + rng.choice(ok, 5).tolist()
    if pattern == "pair":
        body[-1] = tsb + 20  # a lone timestamp: the next token must be a timestamp >= it (or EOS)
    hist = np.asarray(prompt + body, np.int64)
    L = len(hist)
    x = (rng.standard_normal((K + 1, V)) * 3).astype(np.float32)
    if pattern == "mass":
        x[:, tsb:] += 9.0  # timestamps outweigh every text token: the mass rule bans text
    if pattern == "pair":
        x[0, tsb + 20] += 40.0  # the main model closes the pair with the same timestamp
    j_eos = K // 2
    if pattern in ("eos_accepted", "eos_correction"):
        x[j_eos, eos] += 60.0
    max_length = L + max(1, K // 2) if pattern == "maxlen" else L + K + 9
    agree = {"none": 0, "upto": K // 2, "eos_correction": j_eos}.get(pattern, K)
    ids = np.zeros(L + K + 12, np.int64)
    ids[:L] = hist
    for j in range(K):  # sequentially: draft j is position j's token given the drafts before it, or a wrong token
        t = R.greedy_token(ids[: L + j], x[j], gd, P, rt)
        ids[L + j] = t if j < agree else ok[(int(np.searchsorted(ok, t)) + 1 + j) % len(ok)]
        assert j < agree or ids[L + j] != t
    return gd, ids, L, x, max_length


class Case:
    def __init__(self, V, K, rt, gd, ids, L, x, max_length, begin_suppress=True):
        from kwhisper import ops

        dev = "cuda"
        self.K, self.L, self.gd, self.max_length, self.rt = K, L, gd, max_length, rt
        self.host_ids, self.x = ids.copy(), x
        self.logits = torch.from_numpy(x).to(dev)
        sup = torch.zeros(V, dtype=torch.uint8)
        sup[torch.tensor(gd["suppress_tokens"])] = 1
        self.sup = sup.to(dev)
        self.bsup = torch.tensor(gd["begin_suppress_tokens"], dtype=torch.int32, device=dev) if begin_suppress else None
        self.cfg = dict(return_timestamps=rt, ts_begin=gd["no_timestamps_token_id"] + 1,
                        no_ts_id=gd["no_timestamps_token_id"], eos_id=gd["eos_token_id"], pad_id=gd["pad_token_id"],
                        max_initial_ts=gd["max_initial_timestamp_index"] if rt else None, begin_index=P)
        i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)  # noqa: E731
        self.ids = torch.from_numpy(ids)[None].to(dev).contiguous()
        self.cur, self.unf, self.nun = i32([L]), i32([1]), i32([1])
        self.acur, self.aunf, self.vlen, self.stats = i32([L + K + 1]), i32([0]), i32([0]), i32([10, 20, 30])
        self.ws = torch.zeros(ops.spec_accept_workspace_bytes(K) // 4 + 1, device=dev)
        self.accept = ops.SpecAcceptPlan(self.logits, self.sup, self.bsup, self.ids, self.cur, self.unf, self.nun, K=K,
                                         max_length=max_length, workspace=self.ws, asst_cur_len=self.acur,
                                         asst_unfinished=self.aunf, verify_len=self.vlen, stats=self.stats, **self.cfg)

    def greedy_tokens(self):
        """K + 1 sequential kw_greedy_step launches (with a workspace: the split kernels), one per position, each on
        the history with the drafts before it in place."""
        from kwhisper import ops

        dev = "cuda"
        gws = torch.zeros(ops.greedy_step_workspace_bytes(1) // 4 + 1, device=dev)
        toks = []
        for j in range(self.K + 1):
            if self.L + j >= self.max_length:
                toks.append(None)
                continue
            ids = torch.from_numpy(self.host_ids)[None].to(dev).contiguous()
            z = lambda v: torch.tensor([v], dtype=torch.int32, device=dev)  # noqa: E731
            ops.SamplerPlan(self.logits[j: j + 1], self.sup, self.bsup, ids, z(self.L + j), z(1), z(0), z(0), workspace=gws,
                            max_length=self.host_ids.shape[0], **self.cfg)()
            toks.append(int(ids[0, self.L + j].item()))
        return toks

    def state(self):
        torch.cuda.synchronize()
        return dict(ids=self.ids[0].cpu().numpy(), cur=int(self.cur.item()), unf=int(self.unf.item()),
                    nun=int(self.nun.item()), acur=int(self.acur.item()), aunf=int(self.aunf.item()),
                    vlen=int(self.vlen.item()), stats=self.stats.cpu().tolist())

    def check(self, toks):
        want = R.accept(self.host_ids, self.L, self.K, toks, self.gd, self.max_length)
        self.accept()
        got = self.state()
        np.testing.assert_array_equal(got["ids"], want["ids"])
        assert got["cur"] == got["acur"] == want["new_len"] and got["vlen"] == want["new_len"] + self.K
        assert got["unf"] == got["nun"] == int(not want["done"]) and got["aunf"] == 1
        assert got["stats"] == [11, 20 + self.K, 30 + want["n"]]
        assert not self.ws.view(torch.int32).any()  # the workspace is left all zero
        return want, got


@pytest.fixture(params=["torch", "ctypes"])
def backend(request):
    """Every launch of the test -- the accept step and the greedy steps it is held to -- through torch.ops.kw or through
    the ctypes binding of the C ABI."""
    from kwhisper import ops

    old = ops.set_backend(request.param)
    yield request.param
    ops.set_backend(old)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("rt", [False, True])
@pytest.mark.parametrize("V,K", [(V, K) for K in (1, 4, 7) for V in (1000, 51865, 51866)]
                         + [(65545, 4)])  # (V > 65536: the slices' walk beyond their register-held window)
def test_accept_equals_sequential_greedy_steps(V, K, rt, pattern, backend):
    rng = np.random.default_rng(V * 31 + K * 7 + 2 * rt + PATTERNS.index(pattern))
    gd, ids, L, x, max_length = _scenario(V, K, rt, pattern, rng)
    c = Case(V, K, rt, gd, ids, L, x, max_length)
    toks = c.greedy_tokens()
    oracle = R.position_tokens(ids, L, K, x, gd, P, rt, max_length)
    eos = gd["eos_token_id"]
    upto = next((j for j, t in enumerate(oracle) if t == eos or t is None), K)  # (behind an EOS the greedy step pads)
    assert toks[: upto + 1] == oracle[: upto + 1]
    want, got = c.check(toks)
    # the pattern is what it says
    n, done, new_len = want["n"], want["done"], want["new_len"]
    if pattern == "none":
        assert n == 0 and new_len == L + 1
    elif pattern == "all" or (pattern in ("pair", "mass", "first")):
        assert n == K and new_len == L + K + 1 and not done
    elif pattern == "upto":
        assert n == K // 2 and new_len == L + K // 2 + 1 and not done
    elif pattern == "eos_accepted":
        j = K // 2
        assert done and ((n, new_len) == (j + 1, L + j + 1) if j < K else (n, new_len) == (K, L + K + 1))
        assert got["ids"][new_len - 1] == eos and (got["ids"][new_len: L + K + 1] == gd["pad_token_id"]).all()
    elif pattern == "eos_correction":
        assert done and n == K // 2 and got["ids"][new_len - 1] == eos and new_len == L + K // 2 + 1
    elif pattern == "maxlen":
        assert done and new_len == max_length and (got["ids"][max_length:] == ids[max_length:]).all()
    tsb = gd["no_timestamps_token_id"] + 1
    if rt and pattern == "first":
        assert tsb <= got["ids"][L] <= tsb + gd["max_initial_timestamp_index"]
    if rt and pattern == "pair":
        assert got["ids"][L] == tsb + 20 and got["ids"][L + 1] < tsb  # the pair closed: text must follow
    if rt and pattern == "mass":
        assert (got["ids"][L: L + 1] >= tsb).all()


@pytest.mark.parametrize("rt", [False, True])
def test_replay_on_a_finished_row_changes_nothing(rt):
    V, K = 51866, 4
    rng = np.random.default_rng(5 + rt)
    gd, ids, L, x, max_length = _scenario(V, K, rt, "eos_accepted", rng)
    c = Case(V, K, rt, gd, ids, L, x, max_length)
    c.check(c.greedy_tokens())
    first = c.state()
    assert first["unf"] == 0
    c.logits.copy_(torch.from_numpy((rng.standard_normal((K + 1, V)) * 3).astype(np.float32)))
    c.accept()
    c.accept()
    second = c.state()
    np.testing.assert_array_equal(second.pop("ids"), first.pop("ids"))
    assert second == first and not c.ws.view(torch.int32).any()
    # an assistant that drafted on behind the finished row is put back to the final length, nothing else moves
    c.acur.fill_(first["cur"] + K + 1)
    c.accept()
    third = c.state()
    third.pop("ids")
    assert third == first and third["acur"] == third["cur"]


@pytest.mark.parametrize("pattern", ["upto", "first", "mass"])
def test_both_backends_agree(pattern):
    """kw_spec_accept through the ctypes binding of the C ABI (kw_spec_accept_args filled in Python) == through
    torch.ops.kw.spec_accept."""
    from kwhisper import ops

    V, K, rt = 51865, 4, True
    out = {}
    for backend in ("torch", "ctypes"):
        rng = np.random.default_rng(77)
        gd, ids, L, x, max_length = _scenario(V, K, rt, pattern, rng)
        c = Case(V, K, rt, gd, ids, L, x, max_length)
        toks = c.greedy_tokens()
        old = ops.set_backend(backend)
        try:
            c.check(toks)
        finally:
            ops.set_backend(old)
        out[backend] = c.state()
    np.testing.assert_array_equal(out["torch"].pop("ids"), out["ctypes"].pop("ids"))
    assert out["torch"] == out["ctypes"]


def test_no_begin_suppress_and_argument_errors():
    """An empty begin-suppress list (what the paired session passes) at the first position; invalid arguments come
    back as ValueError before any launch."""
    from kwhisper import ops

    V, K, rt = 1000, 4, True
    rng = np.random.default_rng(3)
    gd, ids, L, x, max_length = _scenario(V, K, rt, "first", rng)
    gd = dict(gd, begin_suppress_tokens=None)
    c = Case(V, K, rt, gd, ids, L, x, max_length, begin_suppress=False)
    c.check(c.greedy_tokens())
    with pytest.raises(ValueError):
        ops.SpecAcceptPlan(c.logits, c.sup, None, c.ids, c.cur, c.unf, c.nun, K=K + 1, max_length=max_length,
                           workspace=c.ws, **c.cfg)
    with pytest.raises(ValueError):
        ops.SpecAcceptPlan(c.logits, c.sup, None, c.ids, c.cur, c.unf, c.nun, K=K, max_length=c.ids.shape[1] + 1,
                           workspace=c.ws, **c.cfg)
    with pytest.raises(ValueError):
        ops.SpecAcceptPlan(c.logits, c.sup, None, c.ids, c.cur, c.unf, c.nun, K=K, max_length=max_length,
                           workspace=c.ws[:4], **c.cfg)
