"""Device-resident greedy decoding for one batch (WhisperDecoder + GenerationMixin._sample).

A ``DecodeSession`` owns the static caches and step buffers of one batch:
  * cross K/V of every layer ([2L][B][H][1500][64], one GEMM, TF modeling_whisper.py:323-335), per item
    (beams share it);
  * self K/V static cache [L][B][H][448][64] (replaces DynamicLayer's torch.cat growth,
    TF/cache_utils.py:127-145);
  * ids [B][448] int64, cur_len, unfinished flags -- all on device, advanced by kw_greedy_step.
The prefill (prompt of P tokens) runs eagerly; the single-token step (embedding + 32 x 8 kernels +
LM head with the final LayerNorm fused + sampler) is captured once into a hipGraph (torch.cuda.CUDAGraph) and replayed: the step
reads its position from device memory, so one graph serves every step.  The host only polls the
device unfinished-row count a few steps behind the GPU (no per-step sync).  Graphs are captured with
capture_error_mode="thread_local", so another host thread (another batch in flight on its own stream,
WhisperEngine.lane()) may keep launching while one session captures.  Captures themselves are serialised by one
process-wide lock (``CAPTURE_LOCK``): ``torch.cuda.graph.__enter__`` synchronises the whole device and empties the
allocator cache, which must not run inside another thread's capture; session creation (allocations) takes the same
lock.
"""
from __future__ import annotations

import threading

import numpy as np
import torch

from . import _lib as L
from . import ops

_HD = 64
T_MAX = 448
# serialises every hipGraph capture and every session allocation of the process (lanes capture on host threads)
CAPTURE_LOCK = threading.RLock()


_CAPTURE_STREAMS = {}  # device -> the stream every capture of the process runs on (captures are serialised)


def capture_graph(fn, dev) -> torch.cuda.CUDAGraph:
    """Capture ``fn``'s launches into a new graph on a side stream of its own (L.new_stream: never a pooled stream
    another thread may be launching on), under CAPTURE_LOCK."""
    with CAPTURE_LOCK:
        g = torch.cuda.CUDAGraph()
        key = torch.device(dev).index if torch.device(dev).index is not None else torch.cuda.current_device()
        side = _CAPTURE_STREAMS.get(key)
        if side is None:
            side = _CAPTURE_STREAMS[key] = L.new_stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            fn()
        torch.cuda.current_stream(dev).wait_stream(side)
    return g


class DecodeSession:
    def __init__(self, eng, B: int, enc: torch.Tensor | None = None, beams: int = 1):
        """B batch items decoded as R = B * beams running rows (item-major); cross K/V per item."""
        s = eng.shape
        self.eng, self.B, self.nb = eng, B, beams
        R = self.R = B * beams
        dev, dt = eng.device, eng.dtype
        d, H, Ld = s.d_model, eng.H, s.decoder_layers
        self.T = s.max_source_positions
        # fp8 cross K/V (WhisperEngine(cross_kv_dtype="fp8_e4m3")): e4m3 codes in the bf16 cache's layout and one f32
        # scale per (K/V of a layer, item, head, head dim) instead of the bf16 cache; greedy rows only
        self.fp8 = bool(getattr(eng, "cross_kv_fp8", False))
        if self.fp8 and beams > 1:
            raise NotImplementedError("beam search is not supported with cross_kv_dtype='fp8_e4m3'")
        self.cross = torch.empty((2 * Ld, B, H, self.T, _HD), device=dev, dtype=torch.uint8 if self.fp8 else dt)
        self.cross_scale = torch.empty((2 * Ld, B, H, _HD), device=dev, dtype=torch.float32) if self.fp8 else None
        self.kc = torch.zeros((Ld, R, H, T_MAX, _HD), device=dev, dtype=dt)
        self.vc = torch.zeros((Ld, R, H, T_MAX, _HD), device=dev, dtype=dt)
        self.ids = torch.zeros((R, T_MAX + 1), device=dev, dtype=torch.int64)
        # beam search: cache row holding position p of row r's history (beams share a prefix)
        self.bp = torch.zeros((R, T_MAX), device=dev, dtype=torch.int32) if beams > 1 else None
        self.cur_len = torch.zeros((1,), device=dev, dtype=torch.int32)
        # per-row first key of a left-padded pass (kw_self_attn_step_masked); allocated once: the masked plans and
        # their captured graphs hold its address, generate(key_start=...) fills it per pass
        self.key_start = torch.zeros((R,), device=dev, dtype=torch.int32)
        self._long_q = []  # the long prefill lengths whose buffers are alive, least recently used first
        self.unfinished = torch.ones((R,), device=dev, dtype=torch.int32)
        self.counter = torch.zeros((1,), device=dev, dtype=torch.int32)
        self.n_unfinished = torch.zeros((1,), device=dev, dtype=torch.int32)
        self.logits = torch.empty((R, s.vocab_size), device=dev, dtype=torch.float32)
        self._bufs = {}
        self._plans = {}
        self._align_logs = {}  # alignment pair set -> its query log (token timestamps)
        self.align_out = None  # the last generate(align=...)'s alignment results
        self.keep_alignment = False  # True: align_out also keeps the DTW matrix and the raw weights (validation)
        # split-K seam scratch shared by every decode linear of a step (stream-ordered; zeroed once)
        ws = 0
        if eng.packed:
            for n_, k_ in ((3 * d, d), (d, d), (s.decoder_ffn_dim, d), (d, s.decoder_ffn_dim), (s.vocab_size, d),
                           (H * d, _HD)):
                ws = max(ws, ops.dec_linear_workspace_bytes(n_, k_))
        self.lin_ws = torch.zeros(((ws + 3) // 4,), device=dev, dtype=torch.float32) if ws else None
        self.self_ws = torch.zeros((ops.self_attn_workspace_bytes(R, H, T_MAX) + 3) // 4, device=dev,
                                   dtype=torch.float32)
        # fused self-attention block (kw_dec_qkv_self): greedy rows of the bf16 engine, <= 32 per session, steps
        # at positions < 256 (decided per generate call); its granule workspace is zeroed once, every launch
        # re-arms it
        self.qs_ok = (eng.packed and beams == 1 and eng.fuse_qkv_self and R <= 32
                      and ops.qkv_self_supported(R, d, H))
        self.qs_ws = torch.zeros(((ops.qkv_self_workspace_bytes(R, d) + 3) // 4,), device=dev,
                                 dtype=torch.float32) if self.qs_ok else None
        self.fused_last = False  # whether the last step plan built / replayed used kw_dec_qkv_self
        # fused cross-attention query + step (kw_dec_xq_cross): one query row per item (greedy), any position
        # (over the fp8 cache: kw_dec_xq_cross_fp8, the same workspace and status words)
        self.xc_ok = (eng.packed and beams == 1 and eng.fuse_xq_cross and R <= 32
                      and (ops.xq_cross_fp8_supported if self.fp8 else ops.xq_cross_supported)(R, d, H, self.T))
        self.xc_ws = torch.zeros(((ops.xq_cross_workspace_bytes(R, d, H, self.T) + 3) // 4,), device=dev,
                                 dtype=torch.float32) if self.xc_ok else None
        # fragment-major bf16 residual mirror (KW_LD_TILED) for the q = 1 step: the kernels that read hb there (the
        # self / cross blocks or their LayerNorm-fused projections, fc1, the LM head or kw_dec_lm_greedy) take each
        # fragment as one contiguous 1-KB piece, its producers (embed, o, xo, fc2) write that order -- bitwise the
        # row-major plan.  The fused blocks then write attn in that order too, for o / xo.  Greedy rows of the bf16
        # engine, <= 32 per session, a persistent-LM-head shape.
        self.tiled_ok = bool(eng.packed and beams == 1 and eng.tiled_act and R <= 32 and d % 32 == 0
                             and ops.lm_greedy_supported(R, s.vocab_size, d))
        self._graph = None
        self._graph_key = None
        self._cross_key = None
        # split-row sampler partials + per-row arrival counters (zeroed once; kernels leave them zeroed)
        self.samp_ws = torch.zeros((ops.greedy_step_workspace_bytes(R) + 3) // 4, device=dev, dtype=torch.float32)
        self._greedy_cfg = {}
        self._seq_dev = {}  # sequence_bias / bad_words_ids tables on the device, by content digest
        self._pinned = None
        self._lmg_ws = None  # kw_dec_lm_greedy's partials + arrival counter (zeroed once; launches re-arm it)
        self.lm_greedy_last = False
        self.last_steps = 0
        self._sample_state = None  # kw_sample_step's device scalars and accumulators (made on first use)
        self.avg_logprob = self.n_tokens = None  # per row, left by the last generate(sample=...)
        if enc is not None:
            self.set_encoder_output(enc)

    # ------------------------------------------------------------------------------------------
    def set_encoder_output(self, enc: torch.Tensor, key=None) -> None:
        """Project ``enc`` into every layer's cross K/V.  ``key`` (optional) names the encoder output: a
        repeat call with the key of the K/V already held skips the projection (the v3 multi-task loop
        decodes several prompts against one encoder pass, run_pseudo_labelling_v3.py:309-321)."""
        if key is not None and key == self._cross_key:
            return
        self.eng.cross_kv(enc, self.B, out=(self.cross, self.cross_scale) if self.fp8 else self.cross)
        self._cross_key = key

    def _row_view(self, r0: int, r1: int) -> "DecodeSession":
        """A session over greedy rows [r0, r1) of this one: its ids / caches / cross K/V / logits are row slices
        of this session's, its activation buffers and launch workspaces its own (so two views can run at once).
        Every decode op's per-row arithmetic is independent of the other rows, so a view computes bitwise what
        the full session computes for those rows."""
        v = object.__new__(DecodeSession)
        v.eng, v.nb, v.B, v.R, v.T = self.eng, 1, r1 - r0, r1 - r0, self.T
        v.cross, v.kc, v.vc = self.cross[:, r0:r1], self.kc[:, r0:r1], self.vc[:, r0:r1]
        v.fp8, v.cross_scale = self.fp8, self.cross_scale[:, r0:r1] if self.fp8 else None
        v.ids, v.bp, v.cur_len, v.logits = self.ids[r0:r1], None, self.cur_len, self.logits[r0:r1]
        v.key_start, v._long_q = self.key_start[r0:r1], None  # (a view's long prefill sizes go with its parent's)
        v._bufs, v._plans, v._align_logs = {}, {}, {}
        v.lin_ws = torch.zeros_like(self.lin_ws) if self.lin_ws is not None else None
        v.self_ws = torch.zeros_like(self.self_ws)
        v.qs_ok = v.xc_ok = v.tiled_ok = False
        v.qs_ws = v.xc_ws = None
        return v

    def _prefill_parts(self, parts: int):
        """Row views for a prefill split over ``parts`` side streams (greedy rows only), cached."""
        key = ("views", parts)
        if key not in self._plans:
            R = self.R
            sizes = [R // parts + (1 if i < R % parts else 0) for i in range(parts)]
            views, r0 = [], 0
            for n in sizes:
                views.append(self._row_view(r0, r0 + n))
                r0 += n
            # (streams of their own: a captured prefill forks into them, L.new_stream)
            self._plans[key] = (views, [L.new_stream(self.eng.device, owner=self) for _ in range(parts)])
        return self._plans[key]

    def _run_prefill(self, P: int, parts: int, masked: bool = False) -> None:
        """The prompt's forward pass (prefill) as ``parts`` row blocks on side streams, their launches issued in
        lockstep: each block's kernels are latency-bound chains on few CUs, and two of them overlap (the
        encoder's split, engine._encode_split).  Joined on the current stream before the sampler."""
        if parts <= 1 or self.nb != 1 or self.R < 2 * parts:
            self._run(self._step_plans(P, masked=masked))
            return
        views, streams = self._prefill_parts(parts)
        seqs = [v._step_plans(P, masked=masked) for v in views]
        cur = torch.cuda.current_stream(self.eng.device)
        for st in streams:
            st.wait_stream(cur)
        for j in range(len(seqs[0])):
            for v, seq, st in zip(views, seqs, streams):
                with torch.cuda.stream(st):
                    v._run([seq[j]])
        for st in streams:
            cur.wait_stream(st)

    # Prompts of a few tokens keep one buffer set per length, as ever.  A conditioned pass has a prompt of up to
    # ~228 tokens whose length changes from pass to pass: of those long lengths at most LONG_KEEP stay alive, and a
    # length that leaves takes its plans, its row views' buffers and the configurations whose captured prefill
    # graphs hold its addresses with it -- prefill memory does not grow with the number of lengths seen.
    # Lengths leave only outside a graph capture (generate() and teacher_forced_logits() call _keep_prefill before
    # they capture or run): a dropped configuration destroys its hipGraphs, which is an error inside a capture.
    LONG_Q, LONG_KEEP = 8, 2

    def _keep_prefill(self, q: int) -> None:
        """Mark the long prefill length ``q`` as the most recently used and drop the lengths beyond LONG_KEEP."""
        if q <= self.LONG_Q or self._long_q is None:
            return
        if q in self._long_q:
            self._long_q.remove(q)
        self._long_q.append(q)
        while len(self._long_q) > self.LONG_KEEP:
            self._drop_prefill(self._long_q.pop(0))

    def _drop_prefill(self, q: int) -> None:
        self._bufs.pop(q, None)
        for k in [k for k in self._plans if k[0] == q]:
            del self._plans[k]
        for k in [k for k, c in self._greedy_cfg.items() if c["P"] == q]:
            del self._greedy_cfg[k]
        for k, (views, _) in [(k, v) for k, v in self._plans.items() if k[0] == "views"]:
            for v in views:
                v._bufs.pop(q, None)
                for kk in [kk for kk in v._plans if kk[0] == q]:
                    del v._plans[kk]

    def _buffers(self, q: int):
        if q not in self._bufs:
            if q > self.LONG_Q and self._long_q is not None and q not in self._long_q:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("a long prefill length must be registered (_keep_prefill) before a capture")
                self._keep_prefill(q)
            s, dev, dt = self.eng.shape, self.eng.device, self.eng.dtype
            d, rows = s.d_model, self.R * q
            self._bufs[q] = dict(
                h=torch.empty((rows, d), device=dev, dtype=torch.float32),
                x=torch.empty((rows, d), device=dev, dtype=dt),
                qkv=torch.empty((rows, 3 * d), device=dev, dtype=dt),
                # (q = 1: whole 16-row tiles, zeroed -- the tiled step plan's fused blocks write it fragment-major)
                attn=torch.zeros((16 * ((rows + 15) // 16), d), device=dev, dtype=dt) if q == 1 else
                torch.empty((rows, d), device=dev, dtype=dt),
                qx=torch.empty((rows, d), device=dev, dtype=dt),
                ffn=torch.empty((rows, s.decoder_ffn_dim), device=dev, dtype=dt),
                # cross-attention partials + arrival counters (must start zeroed; kernels leave them zeroed); the fp8
                # cross-attention takes no workspace
                ws=None if self.fp8 else
                torch.zeros((ops.cross_attn_workspace_bytes(self.B, q * self.nb, self.eng.H, _HD, self.T) // 4 + 1,),
                            device=dev, dtype=torch.float32),
            )
            if self.eng.packed:  # bf16 mirror of the residual stream (the LayerNorm-fused linears' operand)
                if q == 1 and self.tiled_ok:  # fragment-major: whole 16-row tiles, rows >= R zero and never written
                    self._bufs[q]["hb"] = torch.zeros((16 * ((rows + 15) // 16), d), device=dev, dtype=torch.bfloat16)
                else:
                    self._bufs[q]["hb"] = torch.empty((rows, d), device=dev, dtype=torch.bfloat16)
        return self._bufs[q]

    def _gemm(self, A, W, C, M, N, K, **kw):
        """f32 parity-mode linear (kw_gemm)."""
        return [ops.GemmPlan(A, W, C, M, N, K, **kw)]

    def _align_log(self, align):
        """The query log [A][R][T_MAX][64] of the alignment pairs ``align``, kept for the session's lifetime: step
        plans and captured graphs hold its address."""
        log = self._align_logs.get(align)
        if log is None:
            log = self._align_logs[align] = torch.zeros((len(align), self.R, T_MAX, _HD), device=self.eng.device,
                                                        dtype=self.eng.dtype)
        return log

    def _step_plans(self, q: int, fused: bool = False, align=None, begin_index: int = 0, masked: bool = False,
                    all_rows: torch.Tensor | None = None):
        """The decoder forward for q new positions per row (q = prompt length for the prefill, 1 after).
        ``all_rows`` (speculative decoding's verify forward): an f32 [R * q][V] buffer; the LM head then runs on every
        one of the q positions into it instead of on the last one into ``self.logits``.  None: exactly the plain plan.
        ``align`` (q == 1): the alignment (layer, head) pairs whose cross-attention queries every step logs
        (kw_align_capture after the layer's query projection; such a layer takes the two-launch cross path, which
        leaves the query in global memory and is bitwise the fused block).  None: exactly the plain plan.
        ``fused`` (q == 1): each layer's LayerNorm-fused QKV projection and self-attention step as ONE
        kw_dec_qkv_self launch (caches bitwise the two-launch plan's, attention within bf16 rounding) -- for steps at positions < 256 only.
        ``masked``: the self-attention items call kw_self_attn_step_masked with this session's ``key_start`` (a
        left-padded pass); there is no masked fused block, so ``fused`` is off."""
        fused = bool(fused and q == 1 and self.qs_ok and not masked)
        key = (q, fused) if align is None else (q, fused, align, begin_index)
        if masked:
            if align is not None:
                raise NotImplementedError("token timestamps with a per-row key_start")
            key = (q, fused, "masked")
        if all_rows is not None:
            if align is not None or masked:
                raise NotImplementedError("an all-rows LM head with token timestamps or a per-row key_start")
            key = (q, fused, "all_rows", all_rows.data_ptr())
        self_kind = "self_masked" if masked else "self"
        if key in self._plans:
            return self._plans[key]
        eng, s = self.eng, self.eng.shape
        b = self._buffers(q)
        capture = {}  # layer -> the capture launch after its cross query projection
        if align is not None:
            log = self._align_log(align)
            for li in sorted({l for l, _ in align}):
                slots = [i for i, (l, _) in enumerate(align) if l == li]
                capture[li] = ops.AlignCapturePlan(b["qx"], [align[i][1] for i in slots], slots, self.cur_len,
                                                   begin_index, log)
        d, H, B = s.d_model, eng.H, self.R  # B: running rows
        rows = B * q
        scale = _HD ** -0.5
        eps = s.layer_norm_eps
        if eng.packed:
            # bf16 path: every decoder LayerNorm is fused into the linear that consumes it
            # (operand = the bf16 residual mirror hb, its rows' statistics computed in that kernel); the
            # residual-add linears update h and hb.
            hb, h = b["hb"], b["h"]
            ws = self.lin_ws
            lin = ops.DecLinearPlan
            tiled = q == 1 and self.tiled_ok  # hb fragment-major (its readers' ldx, its writers' hb_tiled)
            xld = ops.KW_LD_TILED if tiled else None
            seq = [("embed", q, h, hb, tiled)]
            for li, lay in enumerate(eng.dec_layers):
                if fused:
                    seq.append(ops.QkvSelfPlan(hb, lay["qkv_w"], rows, d, H, ln=(eps, lay["qkv_cs"]), bias=lay["qkv_b"],
                                               scale=scale, k_cache=self.kc[li], v_cache=self.vc[li], t_max=T_MAX,
                                               cur_len=self.cur_len, out=b["attn"], workspace=self.qs_ws, ldx=xld))
                else:
                    seq.append(lin(hb, lay["qkv_w"], rows, 3 * d, d, ln=(eps, lay["qkv_cs"]), bias=lay["qkv_b"],
                                   C=b["qkv"], scale=scale, scale_cols=d, workspace=ws, tag="qkv", ldx=xld))
                    seq.append((self_kind, q, b["qkv"], li, b["attn"]))
                seq.append(lin(b["attn"], lay["o_w"], rows, d, d, bias=lay["o_b"], resid=(h, hb, d, 0), workspace=ws,
                               tag="o", hb_tiled=tiled, ldx=xld if fused else None))  # (the fused block's attn)
                xc = q == 1 and self.xc_ok and li not in capture
                if xc and self.fp8:
                    seq.append(ops.XqCrossFp8Plan(hb, lay["xq_w"], rows, d, H, ln=(eps, lay["xq_cs"]), bias=lay["xq_b"],
                                                  scale=scale, k=self.cross[2 * li], v=self.cross[2 * li + 1],
                                                  k_scale=self.cross_scale[2 * li], v_scale=self.cross_scale[2 * li + 1],
                                                  S=self.T, out=b["attn"], workspace=self.xc_ws, ldx=xld))
                elif xc:
                    seq.append(ops.XqCrossPlan(hb, lay["xq_w"], rows, d, H, ln=(eps, lay["xq_cs"]), bias=lay["xq_b"],
                                               scale=scale, k=self.cross[2 * li], v=self.cross[2 * li + 1], S=self.T,
                                               out=b["attn"], workspace=self.xc_ws, ldx=xld))
                else:
                    seq.append(lin(hb, lay["xq_w"], rows, d, d, ln=(eps, lay["xq_cs"]), bias=lay["xq_b"],
                                   C=b["qx"], scale=scale, scale_cols=d, workspace=ws, tag="xq", ldx=xld))
                    if li in capture:
                        seq.append(capture[li])
                    seq.append(("cross", q, b["qx"], li, b["attn"], b["ws"]))
                seq.append(lin(b["attn"], lay["xo_w"], rows, d, d, bias=lay["xo_b"], resid=(h, hb, d, 0),
                               workspace=ws, tag="xo", hb_tiled=tiled, ldx=xld if xc else None))
                seq.append(lin(hb, lay["fc1_w"], rows, s.decoder_ffn_dim, d, ln=(eps, lay["fc1_cs"]),
                               bias=lay["fc1_b"], C=b["ffn"], gelu=True, workspace=ws, tag="fc1", ldx=xld))
                seq.append(lin(b["ffn"], lay["fc2_w"], rows, d, s.decoder_ffn_dim, bias=lay["fc2_b"],
                               resid=(h, hb, d, 0), workspace=ws, tag="fc2", hb_tiled=tiled))
            # final LayerNorm (folded into the packed LM head) + proj_out on the last position of every row
            if all_rows is not None:  # (q > 1 here, so hb is row-major)
                seq.append(lin(hb, eng.lm_w, rows, s.vocab_size, d, ldx=xld, ln=(eps, eng.lm_cs), bias=eng.lm_b,
                               C=all_rows, workspace=ws, tag="lm_head"))
            else:
                seq.append(lin(hb, eng.lm_w, B, s.vocab_size, d, ldx=xld or q * d, x_offset=(q - 1) * d,
                               ln=(eps, eng.lm_cs), bias=eng.lm_b, C=self.logits, workspace=ws, tag="lm_head"))
            self._plans[key] = seq
            return seq
        seq = [("embed", q, b["h"])]
        for li, lay in enumerate(eng.dec_layers):
            seq.append(("ln", b["h"], lay["ln1_g"], lay["ln1_b"], b["x"]))
            seq += self._gemm(b["x"], lay["qkv_w"], b["qkv"], rows, 3 * d, d, bias=lay["qkv_b"], scale=scale,
                              scale_cols=d)
            seq.append((self_kind, q, b["qkv"], li, b["attn"]))
            seq += self._gemm(b["attn"], lay["o_w"], b["h"], rows, d, d, bias=lay["o_b"], epilogue=L.KW_EPI_RESID)
            seq.append(("ln", b["h"], lay["ln2_g"], lay["ln2_b"], b["x"]))
            seq += self._gemm(b["x"], lay["xq_w"], b["qx"], rows, d, d, bias=lay["xq_b"], scale=scale, scale_cols=d)
            if li in capture:
                seq.append(capture[li])
            seq.append(("cross", q, b["qx"], li, b["attn"], b["ws"]))
            seq += self._gemm(b["attn"], lay["xo_w"], b["h"], rows, d, d, bias=lay["xo_b"], epilogue=L.KW_EPI_RESID)
            seq.append(("ln", b["h"], lay["ln3_g"], lay["ln3_b"], b["x"]))
            seq += self._gemm(b["x"], lay["fc1_w"], b["ffn"], rows, s.decoder_ffn_dim, d, bias=lay["fc1_b"],
                              gelu=True)
            seq += self._gemm(b["ffn"], lay["fc2_w"], b["h"], rows, d, s.decoder_ffn_dim, bias=lay["fc2_b"],
                              epilogue=L.KW_EPI_RESID)
        seq.append(("ln", b["h"], eng.dec_ln_g, eng.dec_ln_b, b["x"]))
        # LM head on the last position of every row (proj_out tied to embed_tokens, f32 logits)
        if all_rows is not None:
            seq += self._gemm(b["x"], eng.lm_w, all_rows, rows, s.vocab_size, d)
        else:
            seq += self._gemm(b["x"], eng.lm_w, self.logits, B, s.vocab_size, d, lda=q * d, a_offset=(q - 1) * d)
        self._plans[key] = seq
        return seq

    def _run(self, seq, cur_len: torch.Tensor | None = None):
        """Launch ``seq``.  ``cur_len``: the device length its embedding and self-attention read instead of this
        session's own (speculative decoding's verify forward runs ahead of ``self.cur_len``)."""
        eng, s = self.eng, self.eng.shape
        H, B = eng.H, self.R
        cl = self.cur_len if cur_len is None else cur_len
        for p in seq:
            if not isinstance(p, tuple):
                p()
                continue
            k = p[0]
            if k == "ln":
                ops.layernorm(p[1], p[2], p[3], s.layer_norm_eps, p[4])
            elif k == "embed":
                ops.embed(self.ids, B, p[1], cl, eng.tok_emb, eng.dec_pos, p[2], p[3] if len(p) > 3 else None,
                          hb_tiled=len(p) > 4 and p[4])
            elif k == "self":
                _, q, qkv, li, out = p
                ops.self_attn_step(qkv, B, q, H, _HD, self.kc[li], self.vc[li], T_MAX, cl, out, self.self_ws,
                                   bp=self.bp if q == 1 else None)
            elif k == "self_masked":
                _, q, qkv, li, out = p
                ops.self_attn_step_masked(qkv, B, q, H, _HD, self.kc[li], self.vc[li], T_MAX, cl, self.key_start,
                                          out, self.self_ws, bp=self.bp if q == 1 else None)
            elif k == "cross":  # rows b*nb*q + (beam*q + i) attend to item b's K/V
                _, q, qx, li, out, ws = p
                if self.fp8:
                    ops.cross_attn_step_fp8(qx, self.B, q * self.nb, H, _HD, self.cross[2 * li], self.cross[2 * li + 1],
                                            self.cross_scale[2 * li], self.cross_scale[2 * li + 1], self.T, out)
                else:
                    ops.cross_attn_step(qx, self.B, q * self.nb, H, _HD, self.cross[2 * li], self.cross[2 * li + 1],
                                        self.T, out, ws)

    # ------------------------------------------------------------------------------------------
    def status_words(self):
        """(entry point, workspace, byte offset) of every in-launch hand-off status word this session's launches
        can set (include/kwhisper.h kw_*_status_offset): the fused self block, the fused cross block and the
        unfused cross-attention's combine, one per activation-buffer size."""
        s, H = self.eng.shape, self.eng.H
        out = []
        if self.qs_ws is not None:
            out.append(("kw_dec_qkv_self", self.qs_ws, ops.status_offset("qkv_self", self.R, s.d_model)))
        if self.xc_ws is not None:
            out.append(("kw_dec_xq_cross_fp8" if self.fp8 else "kw_dec_xq_cross", self.xc_ws,
                        ops.status_offset("xq_cross", self.R, s.d_model, H, self.T)))
        for q, b in self._bufs.items():
            if b["ws"] is not None:  # (kw_cross_attn_step_fp8 has no hand-off)
                out.append(("kw_cross_attn_step", b["ws"], ops.status_offset("cross_attn", self.B, q * self.nb, H, _HD,
                                                                             self.T)))
        return out

    def check_handoffs(self) -> None:
        """After the stream is synchronized: raise ``KWError`` if any launch of this session had an in-launch
        hand-off time out (its rows were written as NaN, so its tokens are wrong).  One small device-to-host copy;
        on failure every such workspace is zero-filled (re-armed) first, so the session stays usable."""
        words = self.status_words()
        if not words:
            return
        st = torch.stack([ws.view(torch.int32)[off // 4] for _, ws, off in words]).cpu().tolist()
        bad = [name for (name, _, _), v in zip(words, st) if v != 0]
        if bad:
            for _, ws, _ in words:
                ws.zero_()
            raise L.KWError(f"{', '.join(sorted(set(bad)))}: an in-launch hand-off timed out (a kernel protocol "
                            "failure); the rows it fed are NaN, so this call's tokens are invalid")

    def forward_logits(self, prompt: torch.Tensor) -> torch.Tensor:
        """Prefill only: logits (B, V) for the last prompt position (detect_language)."""
        P = prompt.shape[1]
        self.ids[:, :P].copy_(prompt)
        self.cur_len.fill_(P)
        self._run(self._step_plans(P))
        return self.logits

    def _set_key_start(self, key_start) -> bool:
        """Fill the ``key_start`` buffer for a pass; False (buffer untouched, today's plans) for None or all zero."""
        if key_start is None:
            return False
        ks = np.asarray(key_start, dtype=np.int64).reshape(-1)
        if ks.shape != (self.B,) or (ks < 0).any() or (ks > T_MAX).any():
            raise ValueError(f"key_start must hold one value in [0, {T_MAX}] per row")
        if not ks.any():
            return False
        if self.nb != 1:
            raise NotImplementedError("a per-row key_start with beam search")
        self.key_start.copy_(torch.from_numpy(ks.astype(np.int32)))
        return True

    def teacher_forced_logits(self, seq: torch.Tensor, P: int, key_start=None) -> torch.Tensor:
        """Raw logits (B, T-P+1, V) predicting seq[:, P:] and one more, feeding the reference tokens
        (validation utility: compares the decoder step with a reference's per-step logits).  ``key_start``: per
        row, the first key position attended (a left-padded prompt); None or zeros: the unmasked plans."""
        masked = self._set_key_start(key_start)
        self._keep_prefill(P)
        B, T = seq.shape
        seq = seq.to(self.eng.device)
        self.ids.zero_()
        self.ids[:, :T].copy_(seq)
        self.cur_len.fill_(P)
        out = []
        self._run(self._step_plans(P, masked=masked))
        out.append(self.logits.clone())
        step = self._step_plans(1, fused=T <= 256, masked=masked)
        for t in range(P, T):
            self.cur_len.fill_(t + 1)
            self._run(step)
            out.append(self.logits.clone())
        return torch.stack(out, 1)

    # ------------------------------------------------------------------------------------------
    # the many-row pass: logits of every position of a teacher-forced sequence (model.forward)
    # ------------------------------------------------------------------------------------------
    # bf16 engine: rows (R * T) from which forward_all takes the wide plan (kw_layernorm + kw_gemm over row-major
    # weights) instead of the packed row-chunk plan, whose 32-row chunks stream the weights once per chunk.
    # profiles/distill_forward.txt (large-v3, tools/distill_measure.py), decoder pass in ms, wide / chunk: 64 rows
    # 11.4 / 6.9, 128 rows 12.96 / 12.67, 256 rows 13.5 / 14.7, 1024 rows 14.1 / 27.6, 4096 rows 27.6 / 81.9.  The
    # chunk plan wins up to 128 rows, the wide plan from 256 on; nothing was measured in between, so the threshold is
    # the first size at which the wide plan was seen to win.
    WIDE_MIN_ROWS = 256

    def _wide_plans(self, q: int):
        """bf16 engine: the decoder body for q positions per row on whole-matrix kernels -- per linear a kw_layernorm
        (f32 residual in, bf16 out; gamma / beta are folded into the weights, so it only normalises) and a kw_gemm
        over the row-major weight (q-scale, GELU and the residual add into the f32 stream are its epilogues), the MFMA
        tile prefill self-attention (kw_self_attn_step_masked with this session's all-zero key_start) and the
        cross-attention step.  Ends with the final LayerNorm into the ``x`` buffer; the LM head is the caller's."""
        key = (q, "wide")
        if key in self._plans:
            return self._plans[key]
        eng, s = self.eng, self.eng.shape
        w = eng.wide_weights()
        b = self._buffers(q)
        d, f, rows = s.d_model, s.decoder_ffn_dim, self.R * q
        scale = _HD ** -0.5
        h, x = b["h"], b["x"]
        ln = ("ln", h, w["ln_one"], w["ln_zero"], x)
        gemm, resid = ops.GemmPlan, dict(epilogue=L.KW_EPI_RESID)
        seq = [("embed", q, h)]
        for li, (lay, wl) in enumerate(zip(eng.dec_layers, w["layers"])):
            seq += [ln, gemm(x, wl["qkv_w"], b["qkv"], rows, 3 * d, d, bias=lay["qkv_b"], scale=scale, scale_cols=d),
                    ("self_masked", q, b["qkv"], li, b["attn"]),
                    gemm(b["attn"], wl["o_w"], h, rows, d, d, bias=lay["o_b"], **resid),
                    ln, gemm(x, wl["xq_w"], b["qx"], rows, d, d, bias=lay["xq_b"], scale=scale, scale_cols=d),
                    ("cross", q, b["qx"], li, b["attn"], b["ws"]),
                    gemm(b["attn"], wl["xo_w"], h, rows, d, d, bias=lay["xo_b"], **resid),
                    ln, gemm(x, wl["fc1_w"], b["ffn"], rows, f, d, bias=lay["fc1_b"], gelu=True),
                    gemm(b["ffn"], wl["fc2_w"], h, rows, d, f, bias=lay["fc2_b"], **resid)]
        seq.append(ln)
        self._plans[key] = seq
        return seq

    def _prefill_body(self, q: int):
        """The prefill plan of q positions without its LM head (which reads the last position of every row only):
        everything up to the final residual stream -- on the f32 engine up to the final LayerNorm into ``x``.  The
        head is the plan's last entry; that is checked, not assumed."""
        seq = self._step_plans(q)
        head = seq[-1]
        is_head = getattr(head, "tag", None) == "lm_head" if self.eng.packed else \
            isinstance(head, ops.GemmPlan) and head._keep[2] is self.logits
        if not is_head:
            raise RuntimeError("the prefill plan no longer ends with its LM head")
        return seq[:-1]

    def forward_all(self, ids: torch.Tensor, plan: str | None = None) -> torch.Tensor:
        """Raw f32 logits [R][T][V] of every position of the teacher-forced rows ``ids`` [R][T] (T <= 448), against
        the cross K/V this session holds: the decoder of ``WhisperForConditionalGeneration.forward``
        (TF modeling_whisper.py:690-795, proj_out :1080), no cache kept for a later step.

        f32 engine: the prefill plan (kw_layernorm + kw_gemm) with the LM head on every row.  bf16 engine, ``plan``:
        "chunk" = the packed prefill plan (kw_dec_linear in 32-row chunks), "wide" = ``_wide_plans``; None picks by
        the row count (``WIDE_MIN_ROWS``).  The result is a new tensor every call (of the wide plan: a view of rows
        padded to a multiple of 128 columns); everything else lives in this session's buffers.  Synchronises once, to
        read the in-launch hand-off status words (``check_handoffs``)."""
        eng, s = self.eng, self.eng.shape
        if self.fp8:
            raise NotImplementedError("forward_all over the fp8 cross K/V cache (there is no many-row fp8 "
                                      "cross-attention kernel)")
        if self.nb != 1:
            raise NotImplementedError("forward_all on a beam session")
        if ids.dim() != 2 or ids.shape[0] != self.R or not 1 <= ids.shape[1] <= T_MAX:
            raise ValueError(f"forward_all: ids must be [{self.R}][1 .. {T_MAX}]")
        if plan not in (None, "wide", "chunk") or (plan == "wide" and not eng.packed):
            raise ValueError("forward_all: plan is None, 'chunk' or (bf16 engine) 'wide'")
        R, T = ids.shape
        d, V, rows = s.d_model, s.vocab_size, R * T
        wide = eng.packed and (plan == "wide" or (plan is None and rows >= self.WIDE_MIN_ROWS))
        self.forward_plan_last = "wide" if wide else ("chunk" if eng.packed else "f32")
        self._keep_prefill(T)
        self.ids[:, :T].copy_(ids.to(device=eng.device, dtype=torch.int64))
        self.cur_len.fill_(T)
        if wide:
            w = eng.wide_weights()
            out = torch.empty((rows, w["vpad"]), device=eng.device, dtype=torch.float32)
            self._run(self._wide_plans(T))
            ops.GemmPlan(self._buffers(T)["x"], w["lm_w"], out, rows, w["vpad"], d, bias=w["lm_b"])()
        elif T == 1:  # (the q = 1 step plan keeps its activations fragment-major: its own LM head serves)
            self._run(self._step_plans(1))
            out = self.logits.clone()
        else:
            out = torch.empty((rows, V), device=eng.device, dtype=torch.float32)
            self._run(self._prefill_body(T))
            b = self._buffers(T)
            if eng.packed:
                ops.DecLinearPlan(b["hb"], eng.lm_w, rows, V, d, ln=(s.layer_norm_eps, eng.lm_cs), bias=eng.lm_b, C=out,
                                  workspace=self.lin_ws, tag="lm_head")()
            else:
                ops.GemmPlan(b["x"], eng.lm_w, out, rows, V, d)()
        self.check_handoffs()
        return out.view(R, T, -1)[:, :, :V]

    def _pinned_slots(self, n: int) -> torch.Tensor:
        if self._pinned is None or self._pinned.numel() < n:
            self._pinned = torch.zeros((n,), dtype=torch.int32).pin_memory()
        return self._pinned

    @staticmethod
    def _poll(pinned, events, rep, lag, flag) -> bool:
        """Queue a copy of the device ``flag`` (unfinished rows / beam "go") into pinned slot ``rep % (lag + 1)``
        behind the replay just issued, then read the copy issued ``lag`` replays ago; True once that count is 0
        (every later replay is then a no-op on device: finished rows only append pad).  The slot first gets a -1
        sentinel, so only a count a copy actually delivered can stop the loop (r03al)."""
        slot = rep % (lag + 1)
        pinned[slot] = -1
        pinned[slot: slot + 1].copy_(flag, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        events.append((ev, slot))
        if len(events) > lag:
            e0, s0 = events.pop(0)
            e0.synchronize()
            return int(pinned[s0]) == 0
        return False

    def generate(self, prompt: torch.Tensor, gen, *, max_length: int, return_timestamps: bool,
                 check_every: int = 4, use_graph: bool = True, record_scores: bool = False, align=None,
                 num_frames=None, median_filter_width: int = 7, sample=None, key_start=None, repeat=None,
                 seq_tables=None):
        """Greedy loop of GenerationMixin._sample (TF/generation/utils.py:2783-2941).

        ``sample``: None (the greedy path, unchanged), or a dict -- ``temperature`` (0 = argmax), ``seed``, ``attempt``
        and ``active`` (per-row flags, None = all) -- that selects the statistics path: every step's tail is
        kw_dec_linear(lm) + kw_sample_step (never the fused LM-head + greedy launch), which draws the token at that
        temperature and accumulates each row's log-probability.  The call then leaves ``self.avg_logprob`` (float64) and
        ``self.n_tokens`` per row (_retrieve_avg_logprobs, TF generation_whisper.py:1958-1974).  Inactive rows come back
        as prompt + pad.  Temperature, seed, attempt and the active flags are device scalars, so one captured graph
        serves every attempt of a schedule.

        Returns host int64 ids (B, L) including the prompt, with L exactly the length the reference
        loop stops at (all rows finished or max_length).

        ``align``: the alignment (layer, head) pairs of ``return_token_timestamps``.  Every step then logs those
        heads' cross-attention queries, and after decoding the alignment stage (weights, normalisation, DTW) runs
        on device over the steps the reference would have run; ``self.align_out["frames"]`` holds int32 (B, L - P - 1),
        the encoder position of every step (``num_frames``: per-row feature frames, the crop of
        TF generation_whisper.py:310-354, or None).

        ``key_start``: per row, the number of leading pad positions of a left-padded ``prompt`` (the
        decoder_attention_mask of a conditioned pass, TF generation_whisper.py:1908): the row attends keys from there
        on, positions stay the plain arange.  None or all zero: exactly the unmasked plans and graphs.  Otherwise the
        self-attention runs kw_self_attn_step_masked in the prefill and in every step (never the fused self block).

        ``repeat``: (repetition_penalty, no_repeat_ngram_size), or None.  None or (1.0, 0): exactly today's plans, graph
        keys and launches.  Otherwise kw_repeat_process runs on the raw logits between the LM head and the greedy /
        sampled step -- in the prefill too (the first token is penalised against the prompt) and in every step, on the
        same stream -- so the step's tail is never the fused LM-head + greedy launch.  With ``record_scores`` the
        logits recorded per step are the penalised ones; ``self.raw_logits`` keeps the LM head's own.

        ``seq_tables``: (sequence_bias, bad_words_ids) as ``seq_bias.SeqTable`` or None each, or None.  None / both
        None: exactly today's plans, graph keys and launches.  Otherwise kw_seq_bias_process runs in the same place --
        the sequence_bias table ahead of kw_repeat_process, the bad_words_ids table behind it (TF generation/utils.py:
        1154-1155, 1207-1213) -- in the prefill and in every step, so the tail is never the fused LM-head + greedy
        launch.  The tables' digests are part of the plan / graph key: a captured graph holds the device arrays'
        addresses, and a call with other values gets its own arrays, plans and graphs."""
        repeat = _norm_repeat(repeat)
        seq_dev = self._seq_tables(seq_tables)
        masked = self._set_key_start(key_start)
        self._keep_prefill(prompt.shape[1])
        if masked and align is not None:
            raise NotImplementedError("token timestamps with a per-row key_start")
        if align is not None:
            align = tuple((int(l), int(h)) for l, h in align)
            nl, nh = self.eng.shape.decoder_layers, self.eng.H
            if not align or any(not (0 <= l < nl and 0 <= h < nh) for l, h in align):
                raise ValueError(f"alignment_heads must be [layer, head] pairs within {nl} layers x {nh} heads")
            if self.nb != 1:
                raise NotImplementedError("token timestamps on a beam session go through generate_beam(align=...)")
            if self.fp8:
                raise NotImplementedError("token timestamps with cross_kv_dtype='fp8_e4m3' (kw_align_weights reads the "
                                          "bf16 K cache)")
        self.align_out = None
        B = self.B
        P = prompt.shape[1]
        if P + 1 > T_MAX + 1 or max_length > T_MAX:
            raise ValueError(f"max_length {max_length} exceeds max_target_positions {T_MAX}")
        dev = self.eng.device
        self.ids.zero_()
        self.ids[:, :P].copy_(prompt.to(dev))
        self.cur_len.fill_(P)
        self.unfinished.fill_(1)
        self.counter.zero_()
        self.n_unfinished.fill_(B)
        active = None
        if sample is not None:
            if align is not None or self.nb != 1:
                raise NotImplementedError("sampling / statistics with token timestamps or beam search")
            ss = self._sample_buffers()
            t = float(sample.get("temperature") or 0.0)
            ss["inv_t"].fill_(1.0 / t if t > 0.0 else 0.0)
            seed = int(sample.get("seed", 0)) & 0xFFFFFFFFFFFFFFFF
            ss["seed"].fill_(seed - (1 << 64) if seed >= (1 << 63) else seed)  # (the same 64 bits, as int64)
            att = int(sample.get("attempt", 0)) & 0xFFFFFFFF
            ss["attempt"].fill_(att - (1 << 32) if att >= (1 << 31) else att)
            ss["sum_lp"].zero_()
            ss["n_tok"].zero_()
            active = np.ones(B, bool) if sample.get("active") is None else np.asarray(sample["active"], bool)
            if active.shape != (B,) or not active.any():
                raise ValueError("sample['active'] must flag at least one of the session's rows")
            ss["active"].copy_(torch.from_numpy(active.astype(np.uint8)))
            self.n_unfinished.fill_(int(active.sum()))
        self.avg_logprob = self.n_tokens = None
        # the sampler plan, its processor tables and the captured step graph are kept per configuration:
        # a repeat call (the next batch) replays the same graph (no re-capture)
        key = (max_length, P, bool(return_timestamps), tuple(gen.suppress_tokens or ()),
               tuple(gen.begin_suppress_tokens or ()), gen.timestamp_begin, gen.no_timestamps_token_id,
               gen.eos_token_id, gen.pad_token_id, gen.max_initial_timestamp_index, bool(record_scores),
               self.eng.prefill_streams, self.eng.fuse_lm_greedy, align, "fp8_e4m3" if self.fp8 else None)
        if sample is not None:
            key += ("sample",)
        if masked:
            key += ("masked",)
        if repeat is not None:
            key += (("repeat",) + repeat,)
        if seq_dev is not None:
            key += (("seq",) + tuple(t and t.digest for t in seq_dev),)
        cfg = self._greedy_cfg.get(key)
        if cfg is None:
            sup = torch.zeros((self.eng.shape.vocab_size,), dtype=torch.uint8)
            if gen.suppress_tokens:
                sup[torch.tensor(gen.suppress_tokens)] = 1
            sup = sup.to(dev)
            bsup = torch.tensor(gen.begin_suppress_tokens or [0], dtype=torch.int32, device=dev)
            nb = len(gen.begin_suppress_tokens or [])
            score_buf = torch.empty_like(self.logits) if record_scores and sample is None else None
            pcfg = dict(return_timestamps=return_timestamps, ts_begin=gen.timestamp_begin,
                        no_ts_id=gen.no_timestamps_token_id, eos_id=gen.eos_token_id, pad_id=gen.pad_token_id,
                        max_initial_ts=gen.max_initial_timestamp_index, max_length=max_length, begin_index=P)
            if sample is not None:
                sampler = ops.SamplePlan(self.logits, sup, bsup if nb else None, self.ids, self.cur_len,
                                         self.unfinished, self.counter, self.n_unfinished, inv_temperature=ss["inv_t"],
                                         seed=ss["seed"], attempt=ss["attempt"], sum_logprob=ss["sum_lp"],
                                         n_tokens=ss["n_tok"], active=ss["active"], workspace=ss["ws"], **pcfg)
            else:
                sampler = ops.SamplerPlan(self.logits, sup, bsup if nb else None, self.ids, self.cur_len,
                                          self.unfinished, self.counter, self.n_unfinished, scores_out=score_buf,
                                          workspace=self.samp_ws, **pcfg)
            cfg = dict(sampler=sampler, score_buf=score_buf, graph=None, P=P)
            if repeat is not None:
                cfg["repeat"] = ops.RepeatPlan(self.logits, self.ids, self.cur_len, penalty=repeat[0], ngram=repeat[1])
            if seq_dev is not None:
                cfg["seq"] = tuple(t and ops.SeqBiasPlan(self.logits, self.ids, self.cur_len, t) for t in seq_dev)
            if len(self._greedy_cfg) >= 8:  # bound the cache (each entry may hold a graph)
                self._greedy_cfg.pop(next(iter(self._greedy_cfg)))
            self._greedy_cfg[key] = cfg
        sampler, score_buf = cfg["sampler"], cfg["score_buf"]
        self.scores = [] if record_scores else None
        self.raw_logits = [] if record_scores and (repeat is not None or seq_dev is not None) else None
        rep_plan = cfg.get("repeat")
        sb_plan, bw_plan = cfg.get("seq", (None, None))
        processed = rep_plan is not None or sb_plan is not None or bw_plan is not None

        def processed_tail(tail):
            """The step's token choice, behind the GenerationMixin processors where the call has them: sequence_bias,
            the repetition pair, bad_words_ids."""
            if not processed:
                return tail

            def run():
                if self.raw_logits is not None:
                    self.raw_logits.append(self.logits.clone())
                if sb_plan is not None:
                    sb_plan()
                if rep_plan is not None:
                    rep_plan()
                if bw_plan is not None:
                    bw_plan()
                tail()
            return run

        # prefill (replayed from a graph cached with the configuration: ~260 launches otherwise go
        # through Python one by one)
        first_tail = processed_tail(sampler)

        def prefill():
            self._run_prefill(P, self.eng.prefill_streams, masked)
            first_tail()

        pg = cfg.get("prefill_graph")
        if pg is None and use_graph and not record_scores:
            pg = cfg["prefill_graph"] = capture_graph(prefill, dev)
            # capture only records: the kernels have not run yet, and the state the prefill consumes
            # (ids, cur_len, counters) is untouched -- replay below
        if pg is not None and use_graph and not record_scores:
            pg.replay()
        else:
            prefill()
        if record_scores:
            self.scores.append((self.logits.clone(), score_buf.clone() if score_buf is not None else None))
        n_steps = max_length - P  # tokens the reference can add at most
        done = 1
        fused = max_length <= 256  # every step's position < 256 (kw_dec_qkv_self's key range)
        step_seq = self._step_plans(1, fused=fused, align=align, begin_index=P, masked=masked)
        self.fused_last = bool(fused and self.qs_ok and not masked)
        # the step's LM head + greedy step as one launch (kw_dec_lm_greedy; no timestamps, no recorded scores)
        tail = sampler
        s = self.eng.shape
        if (self.eng.packed and self.nb == 1 and self.eng.fuse_lm_greedy and not return_timestamps and not record_scores
                and sample is None and not processed and ops.lm_greedy_supported(B, s.vocab_size, s.d_model)):
            tail = cfg.get("lm_greedy")
            if tail is None:
                if self._lmg_ws is None:
                    self._lmg_ws = torch.zeros((ops.lm_greedy_workspace_bytes(B, s.vocab_size) + 3) // 4, device=dev,
                                               dtype=torch.float32)
                sa = sampler.args
                tail = cfg["lm_greedy"] = ops.LmGreedyPlan(
                    self._buffers(1)["hb"], self.eng.lm_w, B, s.vocab_size, s.d_model, ln=(s.layer_norm_eps, self.eng.lm_cs),
                    bias=self.eng.lm_b, suppress_mask=sampler._keep[1], begin_suppress=sampler._keep[2], ids=self.ids,
                    cur_len=self.cur_len, unfinished=self.unfinished, n_unfinished=self.n_unfinished, eos_id=sa.eos_id,
                    pad_id=sa.pad_id, max_length=sa.max_length, begin_index=sa.begin_index, workspace=self._lmg_ws,
                    ldx=ops.KW_LD_TILED if self.tiled_ok else None)
            assert getattr(step_seq[-1], "tag", None) == "lm_head"
            step_seq = step_seq[:-1]
        self.lm_greedy_last = tail is not sampler
        tail = processed_tail(tail)

        def one_step():
            self._run(step_seq)
            tail()

        def capture(n):
            def steps():
                for _ in range(n):
                    one_step()
            return capture_graph(steps, dev)

        graph = cfg["graph"]
        if graph is None and use_graph and not record_scores and n_steps > 1:
            graph = cfg["graph"] = capture(1)
        # K (engine.steps_per_replay) steps per replay where K steps remain: one replay launch, unfinished-count
        # copy and event per K steps; every step reads its position from the device, so K steps in one graph are
        # the same K replays of the one-step graph
        K = max(1, int(self.eng.steps_per_replay))
        graph_k = cfg.get(("graph", K)) if K > 1 else None
        if K > 1 and graph_k is None and graph is not None and n_steps > K:
            graph_k = cfg[("graph", K)] = capture(K)
        if not use_graph:
            graph = graph_k = None
        self._graph, self._graph_key = graph, key
        lag = max(1, check_every // K) if graph_k is not None else check_every  # the same lag in steps
        pinned = self._pinned_slots(lag + 1)
        events = []
        rep = 0  # replays issued: slot rep % (lag + 1) is distinct over the lag + 1 copies in flight
        while done < n_steps:
            if graph_k is not None and done + K <= n_steps:
                graph_k.replay()
                done += K
            else:
                if graph is not None:
                    graph.replay()
                else:
                    one_step()
                done += 1
            if record_scores:
                self.scores.append((self.logits.clone(), score_buf.clone() if score_buf is not None else None))
            if self._poll(pinned, events, rep, lag, self.n_unfinished):
                break
            rep += 1
        self.last_steps = done  # steps issued (tests: the stop check fires within lag steps of the last EOS)
        torch.cuda.current_stream(dev).synchronize()  # (this stream only: other lanes keep running)
        self.check_handoffs()
        L_now = int(self.cur_len.item())
        ids = self.ids[:, :L_now].cpu().numpy()
        if sample is not None:
            # the length the reference stops at is that of the rows it decodes: the active ones
            ids = ids[:, : _reference_length(ids[active], P, gen.eos_token_id, max_length).shape[1]]
            n = ss["n_tok"].cpu().numpy().astype(np.int64)
            with np.errstate(invalid="ignore", divide="ignore"):
                self.avg_logprob = ss["sum_lp"].cpu().numpy().astype(np.float64) / n
            self.n_tokens = n
        else:
            ids = _reference_length(ids, P, gen.eos_token_id, max_length)
        if align is not None:
            # the steps the reference ran: one per generated token but the last (not the poll lag's extra replays)
            self.align_out = self._alignment(align, ids.shape[1] - P - 1, num_frames, median_filter_width)
        return ids

    def _sample_buffers(self):
        """kw_sample_step's device scalars (1 / temperature, seed, attempt), per-row accumulators and active flags, and
        its workspace; kept for the session's lifetime (plans and captured graphs hold their addresses)."""
        if self._sample_state is None:
            dev, R = self.eng.device, self.R
            self._sample_state = dict(
                inv_t=torch.zeros((1,), device=dev, dtype=torch.float32),
                seed=torch.zeros((1,), device=dev, dtype=torch.int64),
                attempt=torch.zeros((1,), device=dev, dtype=torch.int32),
                sum_lp=torch.zeros((R,), device=dev, dtype=torch.float32),
                n_tok=torch.zeros((R,), device=dev, dtype=torch.int32),
                active=torch.ones((R,), device=dev, dtype=torch.uint8),
                ws=torch.zeros((ops.sample_step_workspace_bytes(R) + 3) // 4, device=dev, dtype=torch.float32))
        return self._sample_state

    def no_speech_prob(self, sot: int, token: int, logits: torch.Tensor | None = None) -> np.ndarray:
        """softmax of the raw logits at the <|startoftranscript|> position, at ``token`` (<|nospeech|>), per row
        (WhisperNoSpeechDetection, TF generation/logits_process.py:2050-2112); the softmax runs on the device.
        ``logits``: that position's logits if a caller (language detection) already has them."""
        if logits is None:
            logits = self.forward_logits(torch.full((self.B, 1), sot, dtype=torch.int64, device=self.eng.device))
        return torch.softmax(logits.float(), -1)[:, token].cpu().numpy().astype(np.float64)

    def _alignment(self, align, T: int, num_frames, width: int, rows=None):
        """weights -> reduce -> DTW over the first ``T`` logged steps; the host receives (B, T) frame indices.
        ``rows`` (beam search): host int (B, T), the log row -- the running row -- that holds step t of item b
        (kw_align_weights_rows); None: item b's steps are log row b's (kw_align_weights)."""
        B, S, dev = self.B, self.T, self.eng.device
        if T <= 0:
            return dict(frames=np.zeros((B, 0), np.int32), T=0)
        log = self._align_log(align)
        frames = None
        if num_frames is not None:
            # the reference crops with weights[..., : n // 2] (generation_whisper.py:354): a Python slice, so a
            # negative n (a row whose mask ends before the pass's seek) keeps S + n // 2 positions
            frames = torch.tensor([len(range(S)[: int(n) // 2]) for n in num_frames], dtype=torch.int32, device=dev)
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.int32)
            if rows.shape != (B, T) or (rows < 0).any() or (rows >= self.R).any():
                raise ValueError(f"the alignment row table must be (B, T) with entries in [0, {self.R})")
            rows = torch.from_numpy(rows).to(dev)
        A = len(align)
        # pairs per chunk: the f32 weights of a chunk stay under 256 MB (and 32 pairs, the kernels' launch limit)
        chunk = max(1, min(32, A, (256 << 20) // (B * T * S * 4)))
        weights = torch.empty((chunk, B, T, S), device=dev, dtype=torch.float32)
        matrix = torch.empty((B, T, S), device=dev, dtype=torch.float32)
        kept = []
        for a0 in range(0, A, chunk):
            n = min(chunk, A - a0)
            if rows is None:
                ops.align_weights(log, self.cross, align[a0: a0 + n], T, weights, a0=a0, layer_step=2)
            else:
                ops.align_weights_rows(log, rows, self.cross, align[a0: a0 + n], T, weights, a0=a0, layer_step=2)
            ops.align_reduce(weights, n, B, T, S, frames, width, matrix, a_total=A, first=a0 == 0, last=a0 + n >= A)
            if self.keep_alignment:
                kept.append(weights[:n].clone())
        out = ops.dtw(matrix, frames)
        res = dict(frames=out.cpu().numpy(), T=T)
        if self.keep_alignment:
            res["matrix"] = matrix.cpu().numpy()
            res["weights"] = torch.cat(kept).cpu().numpy()  # [A][B][T][S]
            res["num_frames"] = None if frames is None else frames.cpu().numpy()
        return res


    def generate_beam(self, prompt: torch.Tensor, gen, *, num_beams: int, max_length: int, return_timestamps: bool,
                      length_penalty: float = 1.0, early_stopping=False, check_every: int = 4, use_graph: bool = True,
                      repeat=None, align=None, num_frames=None, median_filter_width: int = 7, seq_tables=None):
        """``GenerationMixin._beam_search`` (TF/generation/utils.py:3208-3527) on device, num_return_sequences 1.

        ``prompt`` (B, P) per item.  Returns host int64 (B, P + generated) -- the best finished beam of each
        item, pad-filled, cropped to the batch's longest -- as the reference returns ``sequences``.

        ``repeat``: (repetition_penalty, no_repeat_ngram_size), or None.  None or (1.0, 0): exactly today's plan and
        graphs.  Otherwise kw_beam_logprobs_rep takes kw_beam_logprobs' place: both processors act on every row's
        log-probs, from the row's own re-ordered history, before the Whisper processors.

        ``align``, ``num_frames``, ``median_filter_width``: token timestamps, as in ``generate``.  None: exactly today's
        plan, graph keys and launches.  Otherwise every step logs the alignment heads' queries of all R running rows,
        the selection is kw_beam_select_parents (which also records every step's parents), and after the search the
        host backtraces the returned hypotheses to the reference's ``beam_indices`` (``beam_backtrace``), turns them
        into the row table of TF generation_whisper.py:265-301 (``beam_row_table``) and the alignment stage reads the
        log through it (kw_align_weights_rows).  ``self.align_out`` is laid out as the greedy path's -- ``frames``
        int32 (B, W - 1), W the longest returned hypothesis in generated tokens -- plus ``beam_indices`` (B, W).

        ``seq_tables``: (sequence_bias, bad_words_ids) tables as in ``generate``.  None / both None: exactly today's
        plan and graphs.  Otherwise kw_beam_logprobs_proc is the launch: the bias is added to every row's log-probs
        ahead of the repetition pair, the bad words join the n-gram bans behind it."""
        repeat = _norm_repeat(repeat)
        seq_dev = self._seq_tables(seq_tables)
        B, nb, R = self.B, self.nb, self.R
        if nb != num_beams or nb < 2:
            raise ValueError("session beam width mismatch")
        if align is not None:
            align = tuple((int(l), int(h)) for l, h in align)
            nl, nh = self.eng.shape.decoder_layers, self.eng.H
            if not align or any(not (0 <= l < nl and 0 <= h < nh) for l, h in align):
                raise ValueError(f"alignment_heads must be [layer, head] pairs within {nl} layers x {nh} heads")
        self.align_out = None
        P = prompt.shape[1]
        if max_length > T_MAX:
            raise ValueError(f"max_length {max_length} exceeds max_target_positions {T_MAX}")
        dev = self.eng.device
        V = self.eng.shape.vocab_size
        fill = gen.pad_token_id if gen.pad_token_id is not None else gen.eos_token_id
        self.ids.zero_()
        self.ids[:, :P].copy_(prompt.to(dev).repeat_interleave(nb, 0))
        self.cur_len.fill_(P)
        self.bp.copy_(torch.arange(R, device=dev, dtype=torch.int32)[:, None].expand(R, T_MAX))
        # beam state, step plan and captured graphs are kept per configuration and re-initialised in
        # place, so a repeat call replays the same graphs (no re-capture, see generate)
        key = ("beam", max_length, P, bool(return_timestamps), float(length_penalty), str(early_stopping), fill,
               tuple(gen.suppress_tokens or ()), tuple(gen.begin_suppress_tokens or ()), gen.timestamp_begin,
               gen.no_timestamps_token_id, gen.eos_token_id, gen.max_initial_timestamp_index)
        if repeat is not None:
            key += (("repeat",) + repeat,)
        if seq_dev is not None:
            key += (("seq",) + tuple(t and t.digest for t in seq_dev),)
        if align is not None:
            key += (("align",) + align,)
        cfg = self._greedy_cfg.get(key)
        if cfg is None:
            st = dict(
                ids=self.ids, bp=self.bp, cur_len=self.cur_len,
                run_scores=torch.empty((B * nb,), device=dev, dtype=torch.float32),
                fin_seq=torch.empty((B, nb, max_length), device=dev, dtype=torch.int64),
                fin_score=torch.empty((B, nb), device=dev, dtype=torch.float32),
                fin_len=torch.empty((B, nb), device=dev, dtype=torch.int32),
                fin_flag=torch.empty((B, nb), device=dev, dtype=torch.int32),
                unsat=torch.empty((B,), device=dev, dtype=torch.int32),
                counter=torch.zeros((1,), device=dev, dtype=torch.int32),
                go=torch.empty((1,), device=dev, dtype=torch.int32),
                done=torch.empty((1,), device=dev, dtype=torch.int32),
                item_flags=torch.empty((B, 3), device=dev, dtype=torch.int32),
                cand_val=torch.empty((R, 2 * nb), device=dev, dtype=torch.float32),
                cand_idx=torch.empty((R, 2 * nb), device=dev, dtype=torch.int32),
                lp_ws=torch.zeros(((ops.beam_logprobs_workspace_bytes(R) + 3) // 4,), device=dev, dtype=torch.float32),
            )
            if align is not None:  # (their presence selects kw_beam_select_parents)
                st["parent_log"] = torch.zeros((max_length, R), device=dev, dtype=torch.int32)
                st["fin_parent"] = torch.zeros((B, nb), device=dev, dtype=torch.int32)
            sup = torch.zeros((V,), dtype=torch.uint8)
            if gen.suppress_tokens:
                sup[torch.tensor(gen.suppress_tokens)] = 1
            sup = sup.to(dev)
            bsup = torch.tensor(gen.begin_suppress_tokens or [0], dtype=torch.int32, device=dev)
            step = ops.BeamStepPlan(st, self.logits, sup, bsup if gen.begin_suppress_tokens else None,
                                    return_timestamps=return_timestamps, ts_begin=gen.timestamp_begin,
                                    no_ts_id=gen.no_timestamps_token_id, eos_id=gen.eos_token_id,
                                    max_initial_ts=gen.max_initial_timestamp_index, begin_index=P,
                                    max_length=max_length, fill_id=fill, length_penalty=length_penalty,
                                    early_stopping=early_stopping, repeat=repeat,
                                    **({} if seq_dev is None else {"seq_tables": seq_dev}))
            cfg = dict(st=st, step=step, graph=None, prefill_graph=None, P=P)
            if len(self._greedy_cfg) >= 8:
                self._greedy_cfg.pop(next(iter(self._greedy_cfg)))
            self._greedy_cfg[key] = cfg
        st, step = cfg["st"], cfg["step"]
        st["run_scores"].view(B, nb).fill_(-1.0e9)
        st["run_scores"].view(B, nb)[:, 0] = 0.0
        st["fin_seq"].fill_(fill)
        st["fin_score"].fill_(-1.0e9)
        st["fin_len"].zero_()
        st["fin_flag"].zero_()
        st["unsat"].fill_(1)
        st["counter"].zero_()
        st["go"].fill_(1)
        st["done"].zero_()
        st["item_flags"].zero_()
        if align is not None:
            st["parent_log"].zero_()
            st["fin_parent"].fill_(-1)
        self._beam_state = st

        def prefill():
            self._run(self._step_plans(P))  # prefill on every running row (the reference expands x num_beams)
            step()

        step_seq = self._step_plans(1) if align is None else self._step_plans(1, align=align, begin_index=P)

        def one_step():
            self._run(step_seq)
            step()

        def captured(name, fn):
            g = cfg[name]
            if g is None:
                g = cfg[name] = capture_graph(fn, dev)
            return g

        if use_graph:
            captured("prefill_graph", prefill).replay()
        else:
            prefill()
        graph = captured("graph", one_step) if use_graph else None
        pinned = self._pinned_slots(check_every + 1)
        events = []
        n = 1
        while n < max_length - P + 1:
            if graph is not None:
                graph.replay()
            else:
                one_step()
            if self._poll(pinned, events, n - 1, check_every, st["go"]):
                break
            n += 1
        torch.cuda.current_stream(dev).synchronize()  # (this stream only: other lanes keep running)
        self.check_handoffs()
        fin_len = st["fin_len"][:, 0].cpu().numpy()
        out = st["fin_seq"][:, 0].cpu().numpy()
        if align is not None:
            bi = beam_backtrace(st["parent_log"].cpu().numpy(), st["fin_parent"][:, 0].cpu().numpy(), fin_len, P)
            table = beam_row_table(bi)
            self.align_out = self._alignment(align, table.shape[1], num_frames, median_filter_width, rows=table)
            self.align_out["beam_indices"] = bi
        return out[:, : P + int(fin_len.max())]


    def _seq_tables(self, seq_tables):
        """``seq_tables`` -- (sequence_bias, bad_words_ids) host tables, None each -- as device tables, or None when
        there is neither.  A table goes to the device once per content (its digest) and stays while a plan may hold
        its addresses: the few most recent are kept here, every plan keeps its own besides."""
        if seq_tables is None:
            return None
        sb, bw = seq_tables
        if (sb is None or len(sb) == 0) and (bw is None or len(bw) == 0):
            return None
        V = self.eng.shape.vocab_size
        out = []
        for t in (sb, bw):
            if t is None or len(t) == 0:
                out.append(None)
                continue
            if int(t.tokens.max()) >= V:  # (generate() raises the reference's error before it gets here)
                raise ValueError(f"sequence table token ids must be below the vocabulary size {V}")
            d = self._seq_dev.get(t.digest)
            if d is None:
                if len(self._seq_dev) >= 16:
                    self._seq_dev.pop(next(iter(self._seq_dev)))
                d = self._seq_dev[t.digest] = ops.DeviceSeqTable(t, self.eng.device)
            out.append(d)
        return tuple(out)


def beam_backtrace(parent_log: np.ndarray, fin_parent: np.ndarray, fin_len: np.ndarray, begin_index: int) -> np.ndarray:
    """The reference's ``beam_indices`` of the returned hypotheses from what kw_beam_select_parents recorded.

    ``parent_log`` (max_length, R): row L, written by the step at cur_len = L, names for every next running row the
    running row it continues.  ``fin_parent`` (B,): the running row the returned hypothesis' last token was taken
    from, ``fin_len`` (B,) its generated tokens.  Returns int32 (B, W), W = the longest hypothesis: entry k is the
    running row whose logits gave generated token k, -1 beyond the hypothesis' own length."""
    fin_len = np.asarray(fin_len, dtype=np.int64)
    B, W = len(fin_len), int(fin_len.max()) if len(fin_len) else 0
    out = np.full((B, W), -1, dtype=np.int32)
    for b in range(B):
        n = int(fin_len[b])
        if n == 0:
            continue
        r = int(fin_parent[b])
        out[b, n - 1] = r
        for k in range(n - 1, 0, -1):  # the row that gave token k held, after the step before, the history of ...
            r = int(parent_log[begin_index + k - 1, r])
            out[b, k - 1] = r
    return out


def beam_row_table(beam_indices: np.ndarray) -> np.ndarray:
    """(B, W) ``beam_indices`` -> int32 (B, W - 1): the running row whose cross-attention the reference reads for
    step j of returned row b (TF generation_whisper.py:265-301 once the prompt positions are cut): the row that gave
    token j + 1, and running row 0 of the whole batch where the hypothesis has ended (-1)."""
    bi = np.asarray(beam_indices)
    t = bi[:, 1:].astype(np.int32)
    return np.where(t == -1, 0, t).astype(np.int32)


def _norm_repeat(repeat):
    """``repeat`` as (penalty, ngram) with the values checked, or None when both processors are off."""
    if repeat is None:
        return None
    penalty, ngram = ops.check_repeat(*repeat)
    return None if (penalty == 1.0 and ngram == 0) else (penalty, ngram)


def _reference_length(ids: np.ndarray, P: int, eos: int, max_length: int) -> np.ndarray:
    """Trim to the length at which the reference's while-loop would have stopped."""
    B, L_now = ids.shape
    stop = []
    for b in range(B):
        hit = np.nonzero(ids[b, P:] == eos)[0]
        stop.append(P + int(hit[0]) + 1 if hit.size else max_length)
    L_ref = min(max(stop), max_length, L_now)
    return ids[:, :L_ref]
