"""The decode linears' output bits, pinned: SHA-256 digests of kw_dec_linear / kw_dec_lm_greedy outputs on host-seeded
inputs, recorded from the build before declin.hip's tile steps moved into shared helpers
(tests/golden/declin_parent_digests.json).  A kernel change that is meant to keep every result bit reproduces them.

Inputs come from numpy.random.default_rng on the host and are rounded to bf16 in numpy, so they do not depend on the
torch build; a call the library refuses is pinned as its error code.  One shape per path of choose() / launch_one()
(declin.hip), the geometry (ncb, ktm, nw, ks) read off choose() next to each:

  N   40, K  160  (1,  5, 1, 1)  one wave, partial last column block, element-wise epilogue (N % 16 != 0)
  N   48, K  384  (1,  5, 3, 1)  three waves; 32-row tiles take the spread epilogue with J = 2 jobs
  N   48, K 2592  (1,  5, 6, 3)  K-split seam, 6 waves (81 k-tiles > 80, 27 per split); LayerNorm: KW_EUNSUPPORTED
  N   64, K 2560  (1, 10, 8, 1)  ktm 10 (80 k-tiles in one workgroup), 8 waves -- with so few column groups the 32-row
                                 launch (M <= 16) stages x in LDS, and 80 k-tiles of 32 rows (161 KB) plus the
                                 reduction buffers exceed a workgroup's 160 KB: the runtime refuses those launches
                                 (KW_EHIP, pinned as that); the row split's 16-row chunks (M = 17, 32), a
                                 fragment-major x and the rows kernel (M > 32) run
  N 4112, K 2560  (1, 10, 8, 1)  the same geometry on 257 column groups (no LDS image): every row count runs
  N 5120, K  384  (2,  5, 3, 1)  two column blocks; three waves < J = 4, so 32-row tiles finish on wave 0 and the rows
                                 kernel (M > 32) spreads its four jobs over three waves
  N 5120, K  512  (2,  5, 4, 1)  two column blocks, four waves: the 32-row tile's spread epilogue with J = 4
  N 8192, K  384  (2, 10, 2, 1)  ktm 10 with two column blocks (N >= 8192); LayerNorm f32 here is the LM head
  N 8200, K  256  LM head: 257 column groups, 2 per workgroup, 2 waves -- lm_head_kernel up to 32 rows,
                  lm_head_rows_kernel (8 k-tiles) for 33..320; kw_dec_lm_greedy at B = 3

Rows: 1, 16, 17 (the row split's 16-row chunks wherever 2 * column groups <= CUs: the four narrow shapes), 32, 33 and
70 (rows kernel; K-split: z-chunks), 257 for the K-split shape (a second 32 * ZMAX window); 32 and 40 for the LM shape.

    KW_DECLIN_PIN_RECORD=out.json python -m pytest tests/test_gpu_declin_pin.py   # record instead of assert
"""
import functools
import hashlib
import json
import os
import re

import numpy as np
import pytest
import torch

from kwhisper import _lib as L
from kwhisper import ops

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "declin_parent_digests.json")
RECORD = os.environ.get("KW_DECLIN_PIN_RECORD")
EPS = 1e-5
ROWS = (1, 16, 17, 32, 33, 70)
# name -> (N, K, rows)
SHAPES = {
    "n40_k160": (40, 160, ROWS),
    "n48_k384": (48, 384, ROWS),
    "n48_k2592": (48, 2592, ROWS + (257,)),
    "n64_k2560": (64, 2560, ROWS),
    "n4112_k2560": (4112, 2560, ROWS),
    "n5120_k384": (5120, 384, ROWS),
    "n5120_k512": (5120, 512, ROWS),
    "n8192_k384": (8192, 384, ROWS),
    "lm_n8200_k256": (8200, 256, ROWS + (40,)),
}
MODES = ("resid", "resid_hbt", "ln_f32", "ln_gelu_scale_bf16", "f32", "bf16", "xt_ln_f32", "xt_resid_hbt")
_CODES = {L.KW_EINVAL: "KW_EINVAL", L.KW_EHIP: "KW_EHIP", L.KW_EUNSUPPORTED: "KW_EUNSUPPORTED"}


def _bf16_bits(a):
    """float32 -> bf16 bit patterns (round to nearest even), in numpy."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def _bf16_dev(a):
    return torch.from_numpy(_bf16_bits(a).view(np.int16)).cuda().view(torch.bfloat16)


def _bf16_value(a):
    return (_bf16_bits(a).astype(np.uint32) << 16).view(np.float32)


def _sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def _pinned(fn):
    """fn()'s digest, or the code the library refuses the call with."""
    try:
        out = fn()
        torch.cuda.synchronize()
        return _sha(*out)
    except ValueError:
        return "KW_EINVAL"
    except L.KWError as e:  # ("... failed (code N): ...", _lib.check)
        code = int(re.search(r"code (\d+)", str(e)).group(1))
        if code == L.KW_EHIP:  # a launch the runtime refused leaves HIP's last-error word set: torch's next call
            try:               # reports and clears it
                torch.zeros(1, device="cuda").clone()
                torch.cuda.synchronize()
            except RuntimeError:
                pass
        return _CODES[code]


def _linear(mode, x, xt, Wp, cs, bias, h0, M, N, K, ws):
    xin, ldx = (xt, ops.KW_LD_TILED) if mode.startswith("xt_") else (x, None)
    if "resid" in mode:
        tiled = mode.endswith("hbt")
        h = h0.clone()
        hb = torch.zeros(16 * ((M + 15) // 16) if tiled else M, N, device="cuda", dtype=torch.bfloat16)
        ops.DecLinearPlan(xin, Wp, M, N, K, ldx=ldx, bias=bias, resid=(h, hb, N, 0), workspace=ws, hb_tiled=tiled)()
        return h, hb
    gelu = "gelu" in mode
    C = torch.zeros(M, N, device="cuda", dtype=torch.bfloat16 if mode.endswith("bf16") else torch.float32)
    ops.DecLinearPlan(xin, Wp, M, N, K, ldx=ldx, ln=(EPS, cs) if "ln" in mode else None, bias=bias, C=C, gelu=gelu,
                      scale=0.125 if gelu else 1.0, scale_cols=N // 2 if gelu else 0, workspace=ws)()
    return (C,)


def _shape_digests(name):
    N, K, rows = SHAPES[name]
    rng = np.random.default_rng(sum(name.encode()) * 1000 + N + K)
    w = rng.standard_normal((N, K), dtype=np.float32) / np.float32(K ** 0.5)
    W = _bf16_dev(w)
    cs = torch.from_numpy(_bf16_value(w).astype(np.float64).sum(1).astype(np.float32)).cuda()
    bias = torch.from_numpy(rng.standard_normal(N, dtype=np.float32) * np.float32(0.1)).cuda()
    Wp = ops.pack_weight(W)
    ws = torch.zeros(ops.dec_linear_workspace_bytes(N, K) // 4 + 1, device="cuda")
    out = {}
    for M in rows:
        x = _bf16_dev(rng.standard_normal((M, K), dtype=np.float32) * np.float32(2) + np.float32(0.3))
        h0 = torch.from_numpy(rng.standard_normal((M, N), dtype=np.float32)).cuda()
        xt = ops.act_tile(x) if M <= 32 else None
        modes = ("ln_f32",) if name.startswith("lm_") else MODES
        for mode in modes:
            if M > 32 and (mode.startswith("xt_") or mode.endswith("hbt")):
                continue  # (the fragment-major layouts hold at most two row tiles)
            out[f"{name}/M{M}/{mode}"] = _pinned(functools.partial(_linear, mode, x, xt, Wp, cs, bias, h0, M, N, K, ws))
    if name.startswith("lm_"):
        out.update(_greedy_digests(name, rng, W, Wp, cs, bias, N, K))
    return out


def _greedy_digests(name, rng, W, Wp, cs, bias, V, K, B=3, P=3, steps=4):
    """kw_dec_lm_greedy over a few steps, from row-major and from fragment-major x: ids, cur_len, unfinished,
    n_unfinished and the stored logits.  Row 0 is steered to EOS at the second step (it then emits pad)."""
    eos, pad = 5000, 4999
    sup = np.zeros(V, dtype=np.uint8)
    sup[rng.integers(0, V, 300)] = 1
    sup[eos] = 0
    sup = torch.from_numpy(sup).cuda()
    bsup = torch.tensor([220, eos], dtype=torch.int32, device="cuda")
    xs = [_bf16_dev(rng.standard_normal((B, K), dtype=np.float32) * np.float32(2) + np.float32(0.3))
          for _ in range(steps)]
    xs[1][0] = (W[eos].float() * 8).bfloat16()
    out = {}
    for tiled in (False, True):
        def run():
            ids = torch.zeros((B, 64), dtype=torch.int64, device="cuda")
            ids[:, :P] = torch.tensor([50258, 50266, 50360])
            cur = torch.tensor([P], dtype=torch.int32, device="cuda")
            unf = torch.ones(B, dtype=torch.int32, device="cuda")
            nun = torch.zeros(1, dtype=torch.int32, device="cuda")
            x = torch.zeros(16 * K if tiled else B * K, device="cuda", dtype=torch.bfloat16)
            logits = torch.zeros(B, V, device="cuda")
            gws = torch.zeros(ops.lm_greedy_workspace_bytes(B, V) // 4 + 1, device="cuda")
            plan = ops.LmGreedyPlan(x, Wp, B, V, K, ln=(EPS, cs), bias=bias, suppress_mask=sup, begin_suppress=bsup,
                                    ids=ids, cur_len=cur, unfinished=unf, n_unfinished=nun, eos_id=eos, pad_id=pad,
                                    max_length=P + steps, begin_index=P, workspace=gws, logits=logits,
                                    ldx=ops.KW_LD_TILED if tiled else None)
            logs = []
            for s in xs:
                x.copy_(ops.act_tile(s) if tiled else s.reshape(-1))
                plan()
                logs.append(logits.clone())
            return [ids, cur, unf, nun] + logs
        out[f"{name}/greedy_B{B}/{'xt' if tiled else 'rows'}"] = _pinned(run)
    return out


@functools.lru_cache(maxsize=None)
def _digests(name):
    old = ops.set_backend("ctypes")  # (the C ABI's return codes as they are)
    try:
        return _shape_digests(name)
    finally:
        ops.set_backend(old)


@pytest.mark.parametrize("name", list(SHAPES))
def test_declin_outputs_match_the_recorded_digests(name):
    got = _digests(name)
    if RECORD:
        rec = {}
        if os.path.exists(RECORD):
            with open(RECORD) as f:
                rec = json.load(f)
        rec.update(got)
        with open(RECORD, "w") as f:
            json.dump(rec, f, indent=0, sort_keys=True)
        return
    with open(GOLDEN) as f:
        want = {k: v for k, v in json.load(f).items() if k.startswith(name + "/")}
    assert sorted(got) == sorted(want)
    bad = {k: (got[k][:12], want[k][:12]) for k in got if got[k] != want[k]}
    assert not bad, bad
