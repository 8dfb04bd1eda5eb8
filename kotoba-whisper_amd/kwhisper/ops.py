"""Torch-tensor front end of the kwhisper C ABI, through the PyTorch-ROCm custom ops ``torch.ops.kw.*``.

Every launch goes through a ``torch.ops.kw`` operator (``csrc/torch_ops.cpp``, SURVEY.md §8b: "Torch custom
ops wrap the ABI"), which fills the C ABI's argument block and launches on torch's current HIP stream, so
the kernels are ordinary torch ops to the dispatcher, to ``torch.cuda.graph`` capture and to
``torch.compile`` (fake implementations are registered: every op mutates its outputs and returns nothing).
Tensors are plumbing only (device memory + stream); all arithmetic happens in the HIP kernels of
``libkwhisper.so``.  The plan classes (``GemmPlan``, ``DecLinearPlan``, ``SamplerPlan``, ``SamplePlan``, ``SpecAcceptPlan``, ``RepeatPlan``, ``SeqBiasPlan``, ``BeamStepPlan``)
validate once and keep the op arguments, so decode steps replay without re-validation.

``set_backend("ctypes")`` routes the same calls through the ctypes binding of the C ABI instead (used by
the test that holds the two paths bitwise equal); there is no CPU or torch fallback on either path.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib as L

_DT = {torch.float32: L.KW_DT_F32, torch.bfloat16: L.KW_DT_BF16}
_BACKEND = "torch"


def set_backend(name: str) -> str:
    """Select "torch" (torch.ops.kw, the default) or "ctypes" (the C ABI bound directly); returns the old one."""
    global _BACKEND
    if name not in ("torch", "ctypes"):
        raise ValueError("backend must be 'torch' or 'ctypes'")
    old, _BACKEND = _BACKEND, name
    return old


def backend() -> str:
    return _BACKEND


def _kw():
    """The torch.ops.kw namespace (loads libkwhisper_torch.so once; raises if it is missing)."""
    return L.load_torch_ops()


def _lib():
    return L.load()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _s():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise ValueError(f"unsupported dtype {t.dtype}; expected float32 or bfloat16") from None


def _cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise ValueError("kwhisper ops take device (cuda) tensors")


def _ws_bytes(kind: str, *dims) -> int:
    if _BACKEND == "torch":
        return int(_kw().workspace_bytes(kind, [int(d) for d in dims]))
    fn = {"dec_linear": "kw_dec_linear_workspace_bytes", "packed_weight": "kw_packed_weight_bytes",
          "self_attn": "kw_self_attn_workspace", "cross_attn": "kw_cross_attn_workspace",
          "greedy_step": "kw_greedy_step_workspace", "sample_step": "kw_sample_step_workspace", "beam_logprobs": "kw_beam_logprobs_workspace",
          "lm_greedy": "kw_dec_lm_greedy_workspace", "dtw": "kw_dtw_workspace", "kd_loss": "kw_kd_loss_workspace", "spec_accept": "kw_spec_accept_workspace",
          "qkv_self": "kw_dec_qkv_self_workspace", "xq_cross": "kw_dec_xq_cross_workspace",
          "qkv_self_status": "kw_dec_qkv_self_status_offset", "xq_cross_status": "kw_dec_xq_cross_status_offset",
          "cross_attn_status": "kw_cross_attn_status_offset"}[kind]
    return int(getattr(_lib(), fn)(*dims))


def log_mel(audio: torch.Tensor, mel_filters: torch.Tensor, out: torch.Tensor | None = None,
            workspace: torch.Tensor | None = None) -> torch.Tensor:
    """audio (B, n) f32, n % 160 == 0 -> (B, n_mels, n // 160) f32 log-mel."""
    _cuda(audio, mel_filters)
    if audio.dim() != 2 or audio.dtype != torch.float32 or audio.stride(1) != 1:
        raise ValueError("audio must be a (B, n_samples) float32 tensor with unit inner stride")
    if mel_filters.dim() != 2 or mel_filters.shape[0] != 201 or not mel_filters.is_contiguous():
        raise ValueError("mel_filters must be a contiguous (201, n_mels) float32 tensor")
    b, n = audio.shape
    n_mels = mel_filters.shape[1]
    if out is None:
        out = torch.empty((b, n_mels, n // 160), device=audio.device, dtype=torch.float32)
    if workspace is None:
        workspace = torch.empty((max(b, 1),), device=audio.device, dtype=torch.int32)
    if _BACKEND == "torch":
        _kw().log_mel(audio, mel_filters, out, workspace)
    else:
        L.check(_lib().kw_log_mel(_p(audio), b, n, audio.stride(0), _p(mel_filters), n_mels, _p(out), _p(workspace),
                                  _s()), "kw_log_mel")
    return out


def mel_to_time_major(mel: torch.Tensor, c_pad: int, dtype: torch.dtype, out: torch.Tensor | None = None):
    _cuda(mel)
    b, c, t = mel.shape
    if out is None:
        out = torch.empty((b, t + 2, c_pad), device=mel.device, dtype=dtype)
    mel = mel.contiguous()
    if _BACKEND == "torch":
        _kw().mel_to_time_major(mel, c_pad, out)
    else:
        L.check(_lib().kw_mel_to_time_major(_p(mel), b, c, t, c_pad, _p(out), _DT[dtype], _s()), "kw_mel_to_time_major")
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float, out: torch.Tensor,
              delta: torch.Tensor | None = None):
    """out = LayerNorm(x); with ``delta`` (bf16, x's shape) x += delta first, in place.  x is the residual
    stream: f32 (kw_layernorm) or bf16 (kw_layernorm_bf16res, the sum rounded to bf16)."""
    _cuda(x, gamma, beta, out, delta)
    if x.dtype not in (torch.float32, torch.bfloat16) or not x.is_contiguous():
        raise ValueError("layernorm input must be contiguous float32 or bfloat16")
    if delta is not None and (delta.dtype != torch.bfloat16 or delta.numel() != x.numel() or not delta.is_contiguous()):
        raise ValueError("layernorm delta must be a contiguous bf16 tensor of x's size")
    if _BACKEND == "torch":  # (the operator makes the checks below itself: csrc/torch_ops.cpp)
        _kw().layernorm(x, gamma, beta, float(eps), out, delta)
        return out
    dim = x.shape[-1] if x.dim() else 0
    for t in (gamma, beta):
        if t.dtype != torch.float32 or t.numel() != dim or not t.is_contiguous():
            raise ValueError("layernorm gamma and beta must be contiguous float32 tensors of x's last dimension")
    if out.dtype not in (torch.float32, torch.bfloat16) or out.numel() != x.numel() or not out.is_contiguous():
        raise ValueError("layernorm out must be a contiguous float32 or bfloat16 tensor of x's size")
    if x.numel() == 0:  # no rows: nothing to launch (an empty tensor has no address to pass either)
        return out
    rows = x.numel() // dim
    if x.dtype == torch.bfloat16:
        L.check(_lib().kw_layernorm_bf16res(_p(x), rows, dim, _p(gamma), _p(beta), eps, _p(out), _dt(out), _p(delta),
                                            _s()), "kw_layernorm_bf16res")
    else:
        L.check(_lib().kw_layernorm(_p(x), rows, dim, _p(gamma), _p(beta), eps, _p(out), _dt(out), _p(delta), _s()),
                "kw_layernorm")
    return out


class GemmPlan:
    """A pre-built ``kw_gemm`` call: C = epilogue(A . W^T + bias)."""

    def __init__(self, A, W, C, M, N, K, *, bias=None, lda=None, a_rows_per_batch=0, a_batch_stride=0,
                 ldc=None, c_rows_per_batch=0, c_batch_stride=0, epilogue=L.KW_EPI_STORE, gelu=False,
                 scale=1.0, scale_cols=0, row_add=None, row_add_period=0, hs_seq=0, hs_heads=0, hs_head_dim=0,
                 dtype=None, a_offset=0, c_offset=0):
        _cuda(A, W, C, bias, row_add)
        if bias is not None and bias.dtype != torch.float32:
            raise ValueError("bias must be float32")
        if row_add is not None and row_add.dtype != torch.float32:
            raise ValueError("row_add must be float32")
        lda = K if lda is None else lda
        ldc = N if ldc is None else ldc
        self._keep = (A, W, C, bias, row_add)
        # torch.ops.kw.gemm arguments
        self._geo = [a_offset, lda, a_rows_per_batch, a_batch_stride, c_offset, ldc, c_rows_per_batch, c_batch_stride,
                     M, N, K, epilogue, int(bool(gelu)), scale_cols, row_add_period, hs_seq, hs_heads, hs_head_dim]
        self._targs = (A, W, bias, C, row_add, self._geo, float(scale), -1 if dtype is None else _DT[dtype])
        # the same call as a C argument block (ctypes backend)
        a = L.GemmArgs()
        a.dtype = _dt(W) if dtype is None else _DT[dtype]
        a.c_dtype = _dt(C)
        a.A = A.data_ptr() + a_offset * A.element_size()
        a.lda, a.a_rows_per_batch, a.a_batch_stride = lda, a_rows_per_batch, a_batch_stride
        a.W = W.data_ptr()
        a.bias = bias.data_ptr() if bias is not None else None
        a.C = C.data_ptr() + c_offset * C.element_size()
        a.ldc, a.c_rows_per_batch, a.c_batch_stride = ldc, c_rows_per_batch, c_batch_stride
        a.M, a.N, a.K = M, N, K
        a.epilogue = epilogue
        a.gelu = int(bool(gelu))
        a.scale = float(scale)
        a.scale_cols = scale_cols
        a.row_add = row_add.data_ptr() if row_add is not None else None
        a.row_add_period = row_add_period
        a.hs_seq, a.hs_heads, a.hs_head_dim = hs_seq, hs_heads, hs_head_dim
        self.args = a
        self._ref = ctypes.byref(a)

    def __call__(self):
        if _BACKEND == "torch":
            _kw().gemm(*self._targs)
        else:
            L.check(_lib().kw_gemm(self._ref, _s()), "kw_gemm")


KW_LD_TILED = -1  # a leading dimension that says: this bf16 activation operand is fragment-major (include/kwhisper.h)
KW_EPI_HB_TILED = 0x100  # kw_dec_linear's RESID epilogue writes hb fragment-major
KW_EMBED_HB_TILED = 0x100  # kw_embed writes hb fragment-major


def act_tile(x: torch.Tensor) -> torch.Tensor:
    """[M][K] (M <= 32, K % 32 == 0) -> the fragment-major order the MFMA linears take as ``KW_LD_TILED``: element
    (m, k) is element k % 8 of 16-B piece ((k // 32) * T + m // 16) * 64 + m % 16 + 16 * ((k % 32) // 8), with
    T = ceil(M / 16) row tiles; rows M .. 16 T - 1 are zero.  Flat, (K // 32) * T * 512 elements.  A pure index
    permutation (tests and tools; the engine's producers write the order themselves)."""
    M, K = x.shape
    if not 1 <= M <= 32 or K % 32:
        raise ValueError("act_tile: M <= 32 rows, K % 32 == 0")
    T = (M + 15) // 16
    p = x.new_zeros(16 * T, K)
    p[:M] = x
    # [tile][row][k-tile][piece][8] -> [k-tile][tile][piece][row][8]
    return p.view(T, 16, K // 32, 4, 8).permute(2, 0, 3, 1, 4).contiguous().view(-1)


def act_untile(t: torch.Tensor, M: int, K: int) -> torch.Tensor:
    """The inverse of ``act_tile``: the [M][K] rows of a fragment-major buffer."""
    T = (M + 15) // 16
    return t.view(K // 32, T, 4, 16, 8).permute(1, 3, 0, 2, 4).reshape(16 * T, K)[:M].contiguous()


def dec_linear_workspace_bytes(N: int, K: int) -> int:
    return _ws_bytes("dec_linear", N, K)


class DecLinearPlan:
    """A pre-built ``kw_dec_linear`` call (decode-step linear over packed weights).

    ``x``: bf16 [M][ldx] activations (x_offset elements from the start); ``ln`` = (eps, colsum f32 [N])
    fuses the LayerNorm of x's rows (gamma/beta folded into W/bias by the caller, colsum = row sums of
    the folded bf16 weight: ``ln_colsum``); STORE writes ``C`` (f32 or bf16, ldc); RESID updates
    ``resid`` = (h f32, hb bf16 mirror, ldh, row offset).  ``ldx=KW_LD_TILED``: x is fragment-major (``act_tile``;
    M <= 32); ``hb_tiled``: RESID writes hb fragment-major (KW_EPI_HB_TILED; M <= 32, N % 32 == 0, row offset 0)."""

    def __init__(self, x, W, M, N, K, *, ldx=None, x_offset=0, ln=None, bias=None, C=None, ldc=None, c_offset=0,
                 gelu=False, scale=1.0, scale_cols=0, resid=None, workspace=None, tag=None, hb_tiled=False):
        _cuda(x, W, bias, C, workspace)
        self.tag = tag  # a name for per-kernel timing (bench.py), no effect on the call
        if x.dtype != torch.bfloat16 or W.dtype != torch.bfloat16:
            raise ValueError("kw_dec_linear takes bf16 activations and packed bf16 weights")
        if bias is not None and bias.dtype != torch.float32:
            raise ValueError("bias must be float32")
        ldx = K if ldx is None else ldx
        a = L.DecLinearArgs()
        keep = [x, W, bias, C, workspace]
        a.x = x.data_ptr() + x_offset * 2
        a.ldx = ldx
        colsum, eps = None, 0.0
        if ln is not None:
            eps, colsum = ln
            _cuda(colsum)
            if colsum.dtype != torch.float32 or colsum.numel() < N:
                raise ValueError("ln colsum must be float32 [N]")
            a.ln = 1
            a.ln_eps = float(eps)
            a.ln_colsum = colsum.data_ptr()
            keep.append(colsum)
        a.W = W.data_ptr()
        a.bias = bias.data_ptr() if bias is not None else None
        h = hb = None
        row0 = ldh = 0
        if resid is not None:
            h, hb, ldh, row0 = resid
            _cuda(h, hb)
            if h.dtype != torch.float32 or hb.dtype != torch.bfloat16:
                raise ValueError("RESID needs an f32 residual and a bf16 mirror")
            if hb_tiled and row0:
                raise ValueError("a fragment-major hb takes no row offset")
            a.epilogue = L.KW_EPI_RESID | (KW_EPI_HB_TILED if hb_tiled else 0)
            a.h = h.data_ptr() + row0 * ldh * 4
            a.hb = hb.data_ptr() + row0 * ldh * 2
            a.ldh = ldh
            keep += [h, hb]
            C = None
        else:
            if C is None:
                raise ValueError("STORE needs C")
            if hb_tiled:
                raise ValueError("hb_tiled needs the RESID epilogue")
            a.epilogue = L.KW_EPI_STORE
            ldc = N if ldc is None else ldc
            a.C = C.data_ptr() + c_offset * C.element_size()
            a.ldc = ldc
            a.c_dtype = _dt(C)
        a.gelu = int(bool(gelu))
        a.scale = float(scale)
        a.scale_cols = scale_cols
        a.M, a.N, a.K = M, N, K
        need = dec_linear_workspace_bytes(N, K)
        if workspace is None:
            workspace = torch.zeros((need + 3) // 4, device=W.device, dtype=torch.float32)
            keep.append(workspace)
        if workspace.numel() * workspace.element_size() < need:
            raise ValueError("kw_dec_linear workspace too small")
        a.workspace = workspace.data_ptr()
        a.ws_bytes = workspace.numel() * workspace.element_size()
        self._keep = tuple(keep)
        geo = [x_offset, ldx, 1 if ln is not None else 0, c_offset, 0 if C is None else (ldc or N), int(bool(gelu)),
               scale_cols, row0, ldh, M, N, K] + ([KW_EPI_HB_TILED] if hb_tiled else [])
        self._targs = (x, W, bias, colsum, C, h, hb, workspace, geo, float(eps), float(scale))
        self.args = a
        self._ref = ctypes.byref(a)

    def __call__(self):
        if _BACKEND == "torch":
            _kw().dec_linear(*self._targs)
        else:
            L.check(_lib().kw_dec_linear(self._ref, _s()), "kw_dec_linear")


def ln_colsum(W: torch.Tensor) -> torch.Tensor:
    """f32 [N] row sums of a bf16 [N][K] weight (the values kw_dec_linear multiplies), accumulated in f64."""
    return W.double().sum(1).float().contiguous()


def pack_weight(W: torch.Tensor) -> torch.Tensor:
    """[N][K] bf16 -> packed 16x32-fragment layout for kw_dec_linear."""
    _cuda(W)
    if W.dtype != torch.bfloat16 or W.dim() != 2 or not W.is_contiguous():
        raise ValueError("pack_weight expects a contiguous 2-D bfloat16 tensor")
    n, k = W.shape
    nbytes = _ws_bytes("packed_weight", n, k)
    out = torch.empty((nbytes // 2,), device=W.device, dtype=torch.bfloat16)
    if _BACKEND == "torch":
        _kw().pack_weight(W, out)
    else:
        L.check(_lib().kw_pack_weight(_p(W), n, k, _p(out), _s()), "kw_pack_weight")
    return out


def unpack_weight(packed: torch.Tensor, N: int, K: int, rows: int | None = None) -> torch.Tensor:
    """The inverse of ``pack_weight``: the row-major bf16 [N][K] weight of a packed one (kw_gemm's W operand), as
    ``rows`` >= N rows of which those beyond N are zero.  A pure index permutation, run once per weight: fragment
    (column block cb of 16 rows, k-tile kt) holds, in lane l, the 8 elements k = 32 kt + 8 (l // 16) .. of row
    16 cb + l % 16."""
    _cuda(packed)
    if packed.dtype != torch.bfloat16 or K % 32 or packed.numel() != _ws_bytes("packed_weight", N, K) // 2:
        raise ValueError("unpack_weight expects pack_weight's output for (N, K)")
    cb = packed.numel() // (16 * K)
    w = packed.view(cb, K // 32, 4, 16, 8).permute(0, 3, 1, 2, 4).reshape(cb * 16, K)
    out = torch.zeros((max(N, rows or N), K), device=packed.device, dtype=torch.bfloat16)
    out[:N] = w[:N]
    return out


KW_ATTN_Q_LOG2 = 0x100


def attention(qkv: torch.Tensor, B: int, H: int, T: int, hd: int, out: torch.Tensor, q_log2: bool = False):
    """Encoder self-attention; ``q_log2``: q also carries log2(e) (bf16 only; kw_attention's KW_ATTN_Q_LOG2)."""
    _cuda(qkv, out)
    if qkv.numel() != 3 * B * H * T * hd or out.numel() != B * T * H * hd or qkv.dtype != out.dtype:
        raise ValueError("attention: qkv must hold [3][B][H][T][hd] and out [B][T][H*hd] of one dtype")
    flags = KW_ATTN_Q_LOG2 if q_log2 else 0
    if _BACKEND == "torch":
        _kw().attention(qkv, B, H, T, hd, out, flags)
    else:
        L.check(_lib().kw_attention(_dt(qkv) | flags, _p(qkv), B, H, T, hd, _p(out), _s()), "kw_attention")
    return out


def embed(ids, B, q_len, cur_len, tok_emb, pos_emb, h, hb=None, hb_tiled=False):
    """Decoder embedding into the f32 residual h (and its bf16 mirror hb for the bf16 engine; ``hb_tiled``: written
    fragment-major, KW_EMBED_HB_TILED -- q_len 1, B <= 32)."""
    _cuda(ids, cur_len, tok_emb, pos_emb, h, hb)
    flags = KW_EMBED_HB_TILED if hb_tiled else 0
    if _BACKEND == "torch":
        _kw().embed(ids, B, q_len, cur_len, tok_emb, pos_emb, h, hb, flags)
    else:
        L.check(_lib().kw_embed(_dt(tok_emb) | flags, _p(ids), ids.stride(0), B, q_len, _p(cur_len), _p(tok_emb), _p(pos_emb),
                                tok_emb.shape[1], _p(h), _p(hb), _s()), "kw_embed")


def self_attn_workspace_bytes(B, H, t_max) -> int:
    return _ws_bytes("self_attn", B, H, t_max)


def self_attn_step(qkv, B, q_len, H, hd, k_cache, v_cache, t_max, cur_len, out, workspace=None, bp=None):
    """Static-cache self-attention; q_len == 1 needs a zero-filled ``workspace`` (self_attn_workspace_bytes);
    ``bp``: beam-search slot table [B][>= t_max] int32 (q_len == 1)."""
    _cuda(qkv, k_cache, v_cache, cur_len, out, workspace, bp)
    if _BACKEND == "torch":
        _kw().self_attn_step(qkv, B, q_len, H, hd, k_cache, v_cache, t_max, cur_len, out, workspace, bp)
        return
    nb = workspace.numel() * workspace.element_size() if workspace is not None else 0
    L.check(_lib().kw_self_attn_step(_dt(qkv), _p(qkv), B, q_len, H, hd, _p(k_cache), _p(v_cache), t_max,
                                     _p(cur_len), _p(bp), bp.stride(0) if bp is not None else 0, _p(out),
                                     _p(workspace), nb, _s()), "kw_self_attn_step")


KW_SELF_ATTN_PER_QUERY = 0x100


def self_attn_step_masked(qkv, B, q_len, H, hd, k_cache, v_cache, t_max, cur_len, key_start, out, workspace=None,
                          bp=None, per_query=False):
    """``self_attn_step`` with a per-row first key: row b attends key positions [key_start[b], own position]
    (``key_start``: [B] int32; the keys below are never read; a query below its row's key_start gives zeros).
    ``per_query``: the bf16 prefill by the per-query kernel (the f32 form) instead of the MFMA tile kernel."""
    flags = KW_SELF_ATTN_PER_QUERY if per_query else 0
    _cuda(qkv, k_cache, v_cache, cur_len, key_start, out, workspace, bp)
    if key_start.dtype != torch.int32 or key_start.numel() < B or not key_start.is_contiguous():
        raise ValueError("kw_self_attn_step_masked: key_start must be a contiguous int32 tensor of B elements")
    if _BACKEND == "torch":
        _kw().self_attn_step_masked(qkv, B, q_len, H, hd, k_cache, v_cache, t_max, cur_len, key_start, out, workspace, bp,
                                    flags)
        return
    nb = workspace.numel() * workspace.element_size() if workspace is not None else 0
    L.check(_lib().kw_self_attn_step_masked(_dt(qkv) | flags, _p(qkv), B, q_len, H, hd, _p(k_cache), _p(v_cache), t_max,
                                            _p(cur_len), _p(key_start), _p(bp), bp.stride(0) if bp is not None else 0,
                                            _p(out), _p(workspace), nb, _s()), "kw_self_attn_step_masked")


def qkv_self_workspace_bytes(M, d) -> int:
    return _ws_bytes("qkv_self", M, d)


def qkv_self_supported(M, d, H) -> bool:
    """Whether kw_dec_qkv_self covers the shape (M <= 32, d = 64 H <= 1280)."""
    return bool(_lib().kw_dec_qkv_self_supported(int(M), int(d), int(H)))


class QkvSelfPlan:
    """A pre-built ``kw_dec_qkv_self`` call: LayerNorm-fused QKV projection + self-attention step of one decode
    step in one launch (kw_dec_linear(qkv) then kw_self_attn_step: caches bitwise, attention within bf16 rounding).  ``x``: hb [M][ldx] bf16;
    ``W`` packed (gamma folded), ``ln`` = (eps, colsum [3d]), ``bias`` f32 [3d]; caches one layer's
    [M][H][t_max][64]; ``cur_len`` device int32 (L <= 256); ``out`` attn [M][d] bf16; ``workspace`` zero-filled
    (qkv_self_workspace_bytes).  ``ldx=KW_LD_TILED``: x is read and out written fragment-major (``act_tile``)."""

    def __init__(self, x, W, M, d, H, *, ln, bias, scale, k_cache, v_cache, t_max, cur_len, out, workspace, ldx=None,
                 tag="qkv_self"):
        _cuda(x, W, bias, k_cache, v_cache, cur_len, out, workspace)
        eps, colsum = ln
        _cuda(colsum)
        if x.dtype != torch.bfloat16 or W.dtype != torch.bfloat16 or out.dtype != torch.bfloat16:
            raise ValueError("kw_dec_qkv_self takes bf16 activations, packed bf16 weights and a bf16 output")
        ldx = d if ldx is None else ldx
        if workspace.numel() * workspace.element_size() < qkv_self_workspace_bytes(M, d):
            raise ValueError("kw_dec_qkv_self workspace too small")
        self.tag = tag
        a = L.QkvSelfArgs()
        a.x, a.ldx, a.ln_eps, a.ln_colsum = x.data_ptr(), ldx, float(eps), colsum.data_ptr()
        a.W, a.bias, a.scale = W.data_ptr(), bias.data_ptr() if bias is not None else None, float(scale)
        a.M, a.d, a.H = M, d, H
        a.k_cache, a.v_cache, a.t_max, a.cur_len = k_cache.data_ptr(), v_cache.data_ptr(), t_max, cur_len.data_ptr()
        a.out, a.workspace = out.data_ptr(), workspace.data_ptr()
        a.ws_bytes = workspace.numel() * workspace.element_size()
        self._a = a
        self._ref = ctypes.byref(a)
        self._keep = (x, W, bias, colsum, k_cache, v_cache, cur_len, out, workspace)
        self._targs = (x, W, bias, colsum, k_cache, v_cache, cur_len, out, workspace, [ldx, M, d, H, t_max],
                       float(eps), float(scale))

    def __call__(self):
        if _BACKEND == "torch":
            _kw().dec_qkv_self(*self._targs)
        else:
            L.check(_lib().kw_dec_qkv_self(self._ref, _s()), "kw_dec_qkv_self")


def xq_cross_workspace_bytes(M, d, H, S) -> int:
    return _ws_bytes("xq_cross", M, d, H, S)


def xq_cross_supported(M, d, H, S) -> bool:
    """Whether kw_dec_xq_cross can run here: the shape is one it covers (M <= 32, d = 64 H <= 1280, S whose
    chunks hold 225..256 keys)."""
    return bool(_lib().kw_dec_xq_cross_supported(int(M), int(d), int(H), int(S)))


def cross_attn_pair_kernel(rows, S, fused=False) -> bool:
    """Whether a bf16 one-row cross-attention of ``rows`` (row, head) pairs runs as one workgroup per pair
    (cross_attn_row_kernel) rather than per (pair, chunk) -- kernel naming for profiles; results are equal."""
    return bool(_lib().kw_cross_attn_pair_kernel(int(rows), int(S), int(bool(fused))))


class XqCrossPlan:
    """A pre-built ``kw_dec_xq_cross`` call: the LayerNorm-fused cross-attention query projection and the
    cross-attention step (q_len 1) in one launch (bitwise kw_dec_linear(xq) then kw_cross_attn_step).  ``x``: hb [M][ldx] bf16; ``W`` packed (gamma folded), ``ln`` = (eps, colsum [d]), ``bias``
    f32 [d]; ``k`` / ``v`` one layer's [M][H][S][64]; ``out`` attn [M][d] bf16; ``workspace`` zero-filled
    (xq_cross_workspace_bytes).  ``ldx=KW_LD_TILED``: x is read and out written fragment-major (``act_tile``)."""

    def __init__(self, x, W, M, d, H, *, ln, bias, scale, k, v, S, out, workspace, ldx=None, tag="xq_cross"):
        _cuda(x, W, bias, k, v, out, workspace)
        eps, colsum = ln
        _cuda(colsum)
        if any(t.dtype != torch.bfloat16 for t in (x, W, k, v, out)):
            raise ValueError("kw_dec_xq_cross takes bf16 activations, packed bf16 weights, bf16 K / V and output")
        ldx = d if ldx is None else ldx
        if workspace.numel() * workspace.element_size() < xq_cross_workspace_bytes(M, d, H, S):
            raise ValueError("kw_dec_xq_cross workspace too small")
        self.tag = tag
        a = L.XqCrossArgs()
        a.x, a.ldx, a.ln_eps, a.ln_colsum = x.data_ptr(), ldx, float(eps), colsum.data_ptr()
        a.W, a.bias, a.scale = W.data_ptr(), bias.data_ptr() if bias is not None else None, float(scale)
        a.M, a.d, a.H = M, d, H
        a.k, a.v, a.S = k.data_ptr(), v.data_ptr(), S
        a.out, a.workspace = out.data_ptr(), workspace.data_ptr()
        a.ws_bytes = workspace.numel() * workspace.element_size()
        self._a = a
        self._ref = ctypes.byref(a)
        self._keep = (x, W, bias, colsum, k, v, out, workspace)
        self._targs = (x, W, bias, colsum, k, v, out, workspace, [ldx, M, d, H, S], float(eps), float(scale))

    def __call__(self):
        if _BACKEND == "torch":
            _kw().dec_xq_cross(*self._targs)
        else:
            L.check(_lib().kw_dec_xq_cross(self._ref, _s()), "kw_dec_xq_cross")


def xq_cross_fp8_supported(M, d, H, S) -> bool:
    """Whether kw_dec_xq_cross_fp8 covers the shape (M <= 32, d = 64 H <= 1280, S in six chunks of 225..256 keys)."""
    return bool(_lib().kw_dec_xq_cross_fp8_supported(int(M), int(d), int(H), int(S)))


class XqCrossFp8Plan:
    """A pre-built ``kw_dec_xq_cross_fp8`` call: ``XqCrossPlan`` over the fp8 (e4m3) cross cache -- ``k`` / ``v`` one
    layer's uint8 codes [M][H][S][64], ``k_scale`` / ``v_scale`` its f32 scales [M][H][64]; bitwise kw_dec_linear(xq)
    then kw_cross_attn_step_fp8.  ``workspace``: kw_dec_xq_cross's (xq_cross_workspace_bytes), zero-filled."""

    def __init__(self, x, W, M, d, H, *, ln, bias, scale, k, v, k_scale, v_scale, S, out, workspace, ldx=None,
                 tag="xq_cross_fp8"):
        _cuda(x, W, bias, k, v, k_scale, v_scale, out, workspace)
        eps, colsum = ln
        _cuda(colsum)
        if (any(t.dtype != torch.bfloat16 for t in (x, W, out)) or any(t.dtype != torch.uint8 for t in (k, v))
                or any(t.dtype != torch.float32 for t in (k_scale, v_scale))):
            raise ValueError("kw_dec_xq_cross_fp8 takes bf16 activations, packed bf16 weights, uint8 (e4m3) K / V, f32 "
                             "scales and a bf16 output")
        if not all(t.is_contiguous() for t in (k, v, k_scale, v_scale)):
            raise ValueError("kw_dec_xq_cross_fp8: K / V codes and scales must be contiguous")
        ldx = d if ldx is None else ldx
        if workspace.numel() * workspace.element_size() < xq_cross_workspace_bytes(M, d, H, S):
            raise ValueError("kw_dec_xq_cross_fp8 workspace too small")
        self.tag = tag
        a = L.XqCrossFp8Args()
        a.x, a.ldx, a.ln_eps, a.ln_colsum = x.data_ptr(), ldx, float(eps), colsum.data_ptr()
        a.W, a.bias, a.scale = W.data_ptr(), bias.data_ptr() if bias is not None else None, float(scale)
        a.M, a.d, a.H = M, d, H
        a.k, a.v, a.S = k.data_ptr(), v.data_ptr(), S
        a.k_scale, a.v_scale = k_scale.data_ptr(), v_scale.data_ptr()
        a.out, a.workspace = out.data_ptr(), workspace.data_ptr()
        a.ws_bytes = workspace.numel() * workspace.element_size()
        self._a = a
        self._ref = ctypes.byref(a)
        self._keep = (x, W, bias, colsum, k, v, k_scale, v_scale, out, workspace)
        self._targs = (x, W, bias, colsum, k, v, k_scale, v_scale, out, workspace, [ldx, M, d, H, S], float(eps),
                       float(scale))

    def __call__(self):
        if _BACKEND == "torch":
            _kw().dec_xq_cross_fp8(*self._targs)
        else:
            L.check(_lib().kw_dec_xq_cross_fp8(self._ref, _s()), "kw_dec_xq_cross_fp8")


def cross_kv_quant(x, codes, scales):
    """kw_cross_kv_quant: ``x`` bf16 [..., S, 64] (contiguous; the leading dims are the call's tiles) -> ``codes`` uint8 of
    x's shape (OCP e4m3fn) and ``scales`` f32 [..., 64], the format of include/kwhisper.h "fp8 cross K/V"."""
    _cuda(x, codes, scales)
    if x.dtype != torch.bfloat16 or codes.dtype != torch.uint8 or scales.dtype != torch.float32:
        raise ValueError("kw_cross_kv_quant takes bf16 K / V, uint8 codes and f32 scales")
    if x.dim() < 2 or not (x.is_contiguous() and codes.is_contiguous() and scales.is_contiguous()):
        raise ValueError("kw_cross_kv_quant takes contiguous [..., S, head_dim] tensors")
    S, hd = x.shape[-2], x.shape[-1]
    n = x.numel() // (S * hd)
    if codes.numel() != x.numel() or scales.numel() != n * hd:
        raise ValueError("kw_cross_kv_quant: codes must have x's size and scales one value per (tile, head dim)")
    if _BACKEND == "torch":
        _kw().cross_kv_quant(x, n, S, hd, codes, scales)
        return
    L.check(_lib().kw_cross_kv_quant(_p(x), n, S, hd, _p(codes), _p(scales), _s()), "kw_cross_kv_quant")


def cross_attn_step_fp8(q, B, q_len, H, hd, k, v, k_scale, v_scale, S, out):
    """kw_cross_attn_step_fp8: ``cross_attn_step`` over the fp8 cache (one layer's codes and scales); no workspace."""
    _cuda(q, k, v, k_scale, v_scale, out)
    if not all(t.is_contiguous() for t in (k, v, k_scale, v_scale)):
        raise ValueError("kw_cross_attn_step_fp8: K / V codes and scales must be contiguous")
    if _BACKEND == "torch":
        _kw().cross_attn_step_fp8(q, B, q_len, H, hd, k, v, k_scale, v_scale, S, out)
        return
    if (q.dtype != torch.bfloat16 or out.dtype != torch.bfloat16 or k.dtype != torch.uint8 or v.dtype != torch.uint8
            or k_scale.dtype != torch.float32 or v_scale.dtype != torch.float32):
        raise ValueError("kw_cross_attn_step_fp8 takes a bf16 query and output, uint8 (e4m3) K / V and f32 scales")
    L.check(_lib().kw_cross_attn_step_fp8(_p(q), B, q_len, H, hd, _p(k), _p(v), _p(k_scale), _p(v_scale), S, _p(out),
                                          _s()), "kw_cross_attn_step_fp8")


def cross_attn_workspace_bytes(B, q_len, H, hd, S) -> int:
    return _ws_bytes("cross_attn", B, q_len, H, hd, S)


def status_offset(kind: str, *dims) -> int:
    """Byte offset of the int32 hand-off status word inside the workspace of ``kind`` ("qkv_self",
    "xq_cross", "cross_attn"; the workspace's own dimensions).  The word after it (qkv_self, xq_cross) is the
    fault-injection word (include/kwhisper.h)."""
    return _ws_bytes(f"{kind}_status", *dims)


def cross_attn_step(q, B, q_len, H, hd, k, v, S, out, workspace):
    _cuda(q, k, v, out, workspace)
    if _BACKEND == "torch":
        _kw().cross_attn_step(q, B, q_len, H, hd, k, v, S, out, workspace)
        return
    L.check(_lib().kw_cross_attn_step(_dt(q), _p(q), B, q_len, H, hd, _p(k), _p(v), S, _p(out), _p(workspace),
                                      workspace.numel() * workspace.element_size(), _s()), "kw_cross_attn_step")


def beam_logprobs_workspace_bytes(R: int) -> int:
    return _ws_bytes("beam_logprobs", R)


def greedy_step_workspace_bytes(B: int) -> int:
    return _ws_bytes("greedy_step", B)


class SamplerPlan:
    """Pre-built ``kw_greedy_step`` call (processors + argmax + stopping on device)."""

    def __init__(self, logits, suppress_mask, begin_suppress, ids, cur_len, unfinished, counter, n_unfinished, *,
                 return_timestamps, ts_begin, no_ts_id, eos_id, pad_id, max_initial_ts, max_length, begin_index,
                 scores_out=None, workspace=None):
        _cuda(logits, suppress_mask, begin_suppress, ids, cur_len, unfinished, counter, n_unfinished, scores_out,
              workspace)
        self._keep = (logits, suppress_mask, begin_suppress, ids, cur_len, unfinished, counter, n_unfinished, scores_out,
                      workspace)
        mit = -1 if max_initial_ts is None else max_initial_ts
        cfg = [int(bool(return_timestamps)), ts_begin, no_ts_id, eos_id, pad_id, mit, max_length, begin_index]
        self._targs = (logits, suppress_mask, begin_suppress, ids, cur_len, unfinished, counter, n_unfinished,
                       scores_out, workspace, cfg)
        a = L.SamplerArgs()
        a.logits = logits.data_ptr()
        a.B, a.V = logits.shape
        a.suppress_mask = suppress_mask.data_ptr()
        a.begin_suppress = begin_suppress.data_ptr() if begin_suppress is not None else None
        a.n_begin_suppress = begin_suppress.numel() if begin_suppress is not None else 0
        a.return_timestamps = int(bool(return_timestamps))
        a.ts_begin, a.no_ts_id, a.eos_id, a.pad_id = ts_begin, no_ts_id, eos_id, pad_id
        a.max_initial_ts = mit
        a.ids = ids.data_ptr()
        a.ids_stride = ids.stride(0)
        a.cur_len = cur_len.data_ptr()
        a.max_length = max_length
        a.begin_index = begin_index
        a.unfinished = unfinished.data_ptr()
        a.counter = counter.data_ptr()
        a.n_unfinished = n_unfinished.data_ptr()
        a.scores_out = scores_out.data_ptr() if scores_out is not None else None
        a.workspace = workspace.data_ptr() if workspace is not None else None
        a.ws_bytes = workspace.numel() * workspace.element_size() if workspace is not None else 0
        self.args = a
        self._ref = ctypes.byref(a)

    def __call__(self):
        if _BACKEND == "torch":
            _kw().greedy_step(*self._targs)
        else:
            L.check(_lib().kw_greedy_step(self._ref, _s()), "kw_greedy_step")


def sample_step_workspace_bytes(B: int) -> int:
    return _ws_bytes("sample_step", B)


class SamplePlan:
    """Pre-built ``kw_sample_step`` call: ``SamplerPlan``'s processors, stopping and device state, the token drawn at
    the temperature the device scalar ``inv_temperature`` (f32 [1], 0 = argmax) names with Philox noise keyed by
    ``seed`` (int64 [1]) and ``attempt`` (int32 [1]), and each unfinished row's token log-probability added to
    ``sum_logprob`` (f32 [B]) / ``n_tokens`` (int32 [B]).  ``active`` (uint8 [B], optional): rows with 0 are finished
    from the first step; ``noise_out`` (f32 [B][V], optional): the noise used; ``workspace`` zero-filled
    (sample_step_workspace_bytes)."""

    def __init__(self, logits, suppress_mask, begin_suppress, ids, cur_len, unfinished, counter, n_unfinished, *,
                 inv_temperature, seed, attempt, sum_logprob, n_tokens, workspace, return_timestamps, ts_begin, no_ts_id,
                 eos_id, pad_id, max_initial_ts, max_length, begin_index, active=None, noise_out=None):
        ts = (logits, suppress_mask, begin_suppress, ids, cur_len, unfinished, counter, n_unfinished, inv_temperature,
              seed, attempt, sum_logprob, n_tokens, active, noise_out, workspace)
        _cuda(*ts)
        B, V = logits.shape
        if logits.dtype != torch.float32 or not logits.is_contiguous():
            raise ValueError("kw_sample_step takes contiguous float32 logits")
        if (inv_temperature.dtype != torch.float32 or seed.dtype != torch.int64 or attempt.dtype != torch.int32
                or sum_logprob.dtype != torch.float32 or n_tokens.dtype != torch.int32 or sum_logprob.numel() < B
                or n_tokens.numel() < B):
            raise ValueError("kw_sample_step: inv_temperature f32 [1], seed int64 [1], attempt int32 [1], sum_logprob "
                             "f32 [B], n_tokens int32 [B]")
        if active is not None and (active.dtype != torch.uint8 or active.numel() < B):
            raise ValueError("kw_sample_step: active must be uint8 [B]")
        if noise_out is not None and (noise_out.dtype != torch.float32 or not noise_out.is_contiguous()
                                      or noise_out.numel() < B * V):
            raise ValueError("kw_sample_step: noise_out must be a contiguous float32 [B][V] tensor")
        if (suppress_mask.numel() < V or unfinished.numel() < B or ids.shape[0] < B or ids.stride(1) != 1
                or ids.shape[1] < max_length):
            raise ValueError("kw_sample_step: suppress_mask [V], unfinished [B], ids [B][>= max_length]")
        if workspace.numel() * workspace.element_size() < sample_step_workspace_bytes(B):
            raise ValueError("kw_sample_step workspace too small")
        self._keep = ts
        mit = -1 if max_initial_ts is None else max_initial_ts
        cfg = [int(bool(return_timestamps)), ts_begin, no_ts_id, eos_id, pad_id, mit, max_length, begin_index]
        self._targs = (logits, suppress_mask, begin_suppress, ids, cur_len, unfinished, counter, n_unfinished,
                       inv_temperature, seed, attempt, sum_logprob, n_tokens, active, noise_out, workspace, cfg)
        a = L.SampleArgs()
        a.logits = logits.data_ptr()
        a.B, a.V = B, V
        a.suppress_mask = suppress_mask.data_ptr()
        a.begin_suppress = begin_suppress.data_ptr() if begin_suppress is not None else None
        a.n_begin_suppress = begin_suppress.numel() if begin_suppress is not None else 0
        a.return_timestamps = int(bool(return_timestamps))
        a.ts_begin, a.no_ts_id, a.eos_id, a.pad_id = ts_begin, no_ts_id, eos_id, pad_id
        a.max_initial_ts = mit
        a.ids, a.ids_stride, a.cur_len = ids.data_ptr(), ids.stride(0), cur_len.data_ptr()
        a.max_length, a.begin_index = max_length, begin_index
        a.unfinished, a.counter, a.n_unfinished = unfinished.data_ptr(), counter.data_ptr(), n_unfinished.data_ptr()
        a.inv_temperature, a.seed, a.attempt = inv_temperature.data_ptr(), seed.data_ptr(), attempt.data_ptr()
        a.sum_logprob, a.n_tokens = sum_logprob.data_ptr(), n_tokens.data_ptr()
        a.active = active.data_ptr() if active is not None else None
        a.noise_out = noise_out.data_ptr() if noise_out is not None else None
        a.workspace, a.ws_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
        self.args = a
        self._ref = ctypes.byref(a)

    def __call__(self):
        if _BACKEND == "torch":
            _kw().sample_step(*self._targs)
        else:
            L.check(_lib().kw_sample_step(self._ref, _s()), "kw_sample_step")


SPEC_K_MAX = 31  # kw_spec_accept: K + 1 <= 32 positions per launch


def spec_accept_workspace_bytes(K: int) -> int:
    return _ws_bytes("spec_accept", K)


class SpecAcceptPlan:
    """Pre-built ``kw_spec_accept`` call: the accept step of one speculative-decoding round, for one row.  ``logits``:
    f32 [K + 1][V], the main decoder's logits of positions L .. L + K (L = ``*cur_len``); ``ids``: the row (int64, 1-D
    or row 0 of a 2-D tensor) with the K drafts at [L, L + K).  Every position's token is ``SamplerPlan``'s at that
    length; the longest agreeing prefix is kept, then the correction or the bonus token.  Writes ``cur_len``,
    ``unfinished``, ``n_unfinished`` and, where given, ``asst_cur_len`` (= the new length), ``asst_unfinished`` (= 1),
    ``verify_len`` (= the new length + K) and ``stats`` (int32 [3]: rounds, drafted, accepted -- added to).
    ``workspace`` zero-filled (spec_accept_workspace_bytes); every launch leaves it zeroed."""

    def __init__(self, logits, suppress_mask, begin_suppress, ids, cur_len, unfinished, n_unfinished, *, K,
                 return_timestamps, ts_begin, no_ts_id, eos_id, pad_id, max_initial_ts, max_length, begin_index, workspace,
                 asst_cur_len=None, asst_unfinished=None, verify_len=None, stats=None):
        ts = (logits, suppress_mask, begin_suppress, ids, cur_len, unfinished, n_unfinished, asst_cur_len, asst_unfinished,
              verify_len, stats, workspace)
        _cuda(*ts)
        K = int(K)
        if not 1 <= K <= SPEC_K_MAX:
            raise ValueError(f"kw_spec_accept: K must be in [1, {SPEC_K_MAX}]")
        if logits.dim() != 2 or logits.dtype != torch.float32 or not logits.is_contiguous() or logits.shape[0] != K + 1:
            raise ValueError("kw_spec_accept: logits must be a contiguous (K + 1, V) float32 tensor")
        V = logits.shape[1]
        for t, n in ((cur_len, 1), (unfinished, 1), (n_unfinished, 1), (asst_cur_len, 1), (asst_unfinished, 1),
                     (verify_len, 1), (stats, 3)):
            if t is not None and (t.dtype != torch.int32 or t.numel() < n):
                raise ValueError("kw_spec_accept: cur_len, unfinished, n_unfinished, asst_cur_len, asst_unfinished, "
                                 "verify_len int32 [1], stats int32 [3]")
        if (ids.dtype != torch.int64 or ids.stride(-1) != 1 or ids.shape[-1] < max_length
                or suppress_mask.dtype != torch.uint8 or suppress_mask.numel() < V):
            raise ValueError("kw_spec_accept: ids int64 [>= max_length], suppress_mask uint8 [V]")
        if workspace.numel() * workspace.element_size() < spec_accept_workspace_bytes(K):
            raise ValueError("kw_spec_accept workspace too small")
        self._keep = ts
        mit = -1 if max_initial_ts is None else max_initial_ts
        cfg = [int(bool(return_timestamps)), ts_begin, no_ts_id, eos_id, pad_id, mit, max_length, begin_index, K]
        self._targs = (logits, suppress_mask, begin_suppress, ids, cur_len, unfinished, n_unfinished, asst_cur_len,
                       asst_unfinished, verify_len, stats, workspace, cfg)
        a = L.SpecAcceptArgs()
        a.logits, a.V, a.K = logits.data_ptr(), V, K
        a.suppress_mask = suppress_mask.data_ptr()
        a.begin_suppress = begin_suppress.data_ptr() if begin_suppress is not None else None
        a.n_begin_suppress = begin_suppress.numel() if begin_suppress is not None else 0
        a.return_timestamps = int(bool(return_timestamps))
        a.ts_begin, a.no_ts_id, a.eos_id, a.pad_id = ts_begin, no_ts_id, eos_id, pad_id
        a.max_initial_ts = mit
        a.ids, a.ids_stride, a.cur_len = ids.data_ptr(), ids.shape[-1], cur_len.data_ptr()
        a.max_length, a.begin_index = max_length, begin_index
        a.unfinished, a.n_unfinished = unfinished.data_ptr(), n_unfinished.data_ptr()
        a.asst_cur_len = asst_cur_len.data_ptr() if asst_cur_len is not None else None
        a.asst_unfinished = asst_unfinished.data_ptr() if asst_unfinished is not None else None
        a.verify_len = verify_len.data_ptr() if verify_len is not None else None
        a.stats = stats.data_ptr() if stats is not None else None
        a.workspace, a.ws_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
        self.args = a
        self._ref = ctypes.byref(a)

    def __call__(self):
        if _BACKEND == "torch":
            _kw().spec_accept(*self._targs)
        else:
            L.check(_lib().kw_spec_accept(self._ref, _s()), "kw_spec_accept")


def lm_greedy_workspace_bytes(B: int, V: int) -> int:
    return _ws_bytes("lm_greedy", B, V)


def lm_greedy_supported(B: int, V: int, d: int) -> bool:
    """Whether kw_dec_lm_greedy covers the shape (B <= 32 rows, the persistent LM head's geometry)."""
    return bool(_lib().kw_dec_lm_greedy_supported(int(B), int(V), int(d)))


class LmGreedyPlan:
    """A pre-built ``kw_dec_lm_greedy`` call: the LM head (final LayerNorm folded, as the ``DecLinearPlan`` with
    ``ln`` it replaces) and the greedy step without timestamps (as ``SamplerPlan``) in one launch.  ``x``: hb
    [M][ldx] bf16 (x_offset elements in); ``logits``: optional f32 [M][V] (None: not stored); ``workspace``
    zero-filled (lm_greedy_workspace_bytes); the device state (ids, cur_len, unfinished, n_unfinished) is the
    sampler's."""

    def __init__(self, x, W, M, N, K, *, ln, bias, suppress_mask, begin_suppress, ids, cur_len, unfinished,
                 n_unfinished, eos_id, pad_id, max_length, begin_index, workspace, logits=None, ldx=None, x_offset=0,
                 tag="lm_greedy"):
        eps, colsum = ln
        _cuda(x, W, bias, colsum, logits, suppress_mask, begin_suppress, ids, cur_len, unfinished, n_unfinished,
              workspace)
        if x.dtype != torch.bfloat16 or W.dtype != torch.bfloat16:
            raise ValueError("kw_dec_lm_greedy takes bf16 activations and packed bf16 weights")
        if workspace.numel() * workspace.element_size() < lm_greedy_workspace_bytes(M, N):
            raise ValueError("kw_dec_lm_greedy workspace too small")
        ldx = K if ldx is None else ldx
        self.tag = tag
        a = L.DecLinearArgs()
        a.x, a.ldx, a.ln, a.ln_eps, a.ln_colsum = x.data_ptr() + x_offset * 2, ldx, 1, float(eps), colsum.data_ptr()
        a.W, a.bias = W.data_ptr(), bias.data_ptr() if bias is not None else None
        a.epilogue, a.C, a.ldc, a.c_dtype = L.KW_EPI_STORE, _p(logits), logits.stride(0) if logits is not None else N, L.KW_DT_F32
        a.scale, a.M, a.N, a.K = 1.0, M, N, K
        g = L.SamplerArgs()
        g.B, g.V = M, N
        g.suppress_mask = suppress_mask.data_ptr()
        g.begin_suppress = begin_suppress.data_ptr() if begin_suppress is not None else None
        g.n_begin_suppress = begin_suppress.numel() if begin_suppress is not None else 0
        g.eos_id, g.pad_id, g.max_length, g.begin_index, g.max_initial_ts = eos_id, pad_id, max_length, begin_index, -1
        g.ids, g.ids_stride, g.cur_len = ids.data_ptr(), ids.stride(0), cur_len.data_ptr()
        g.unfinished, g.n_unfinished = unfinished.data_ptr(), n_unfinished.data_ptr()
        g.workspace, g.ws_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
        self._a, self._g = a, g
        self._ra, self._rg = ctypes.byref(a), ctypes.byref(g)
        self._keep = (x, W, bias, colsum, logits, suppress_mask, begin_suppress, ids, cur_len, unfinished, n_unfinished,
                      workspace)
        self._targs = (x, W, bias, colsum, logits, suppress_mask, begin_suppress, ids, cur_len, unfinished, n_unfinished,
                       workspace, [x_offset, ldx, M, N, K], float(eps), [eos_id, pad_id, max_length, begin_index])

    def __call__(self):
        if _BACKEND == "torch":
            _kw().dec_lm_greedy(*self._targs)
        else:
            L.check(_lib().kw_dec_lm_greedy(self._ra, self._rg, _s()), "kw_dec_lm_greedy")


def check_repeat(penalty, ngram):
    """(penalty as the f32 the kernels take, ngram) of a ``repeat`` pair; ValueError as the entry points' KW_EINVAL."""
    penalty, ngram = float(penalty), int(ngram)
    if not (penalty > 0.0) or penalty == float("inf") or ngram < 0 or ngram > 0x7fffffff:
        raise ValueError("repeat: penalty must be a finite float > 0 and ngram an int >= 0")
    return penalty, ngram


class RepeatPlan:
    """Pre-built ``kw_repeat_process`` call: repetition_penalty (1.0 = off) and no_repeat_ngram_size (0 = off) in place
    on the f32 ``scores`` [R][V], from every row's history ``ids[r][0 .. *cur_len)`` (the device scalar, so a captured
    step replays).  Runs between the LM head and ``SamplerPlan`` / ``SamplePlan``."""

    def __init__(self, scores, ids, cur_len, *, penalty, ngram):
        _cuda(scores, ids, cur_len)
        penalty, ngram = check_repeat(penalty, ngram)
        if scores.dim() != 2 or scores.dtype != torch.float32 or not scores.is_contiguous():
            raise ValueError("kw_repeat_process: scores must be a contiguous (R, V) float32 tensor")
        if (ids.dim() != 2 or ids.dtype != torch.int64 or ids.stride(1) != 1 or ids.shape[0] < scores.shape[0]
                or cur_len.dtype != torch.int32 or cur_len.numel() < 1):
            raise ValueError("kw_repeat_process: ids int64 [R][ids_stride], cur_len int32 [1]")
        self._keep = (scores, ids, cur_len)
        self._targs = (scores, ids, cur_len, penalty, ngram)
        R, V = scores.shape
        self._cargs = (scores.data_ptr(), R, V, ids.data_ptr(), ids.stride(0), cur_len.data_ptr(), penalty, ngram)

    def __call__(self):
        if _BACKEND == "torch":
            _kw().repeat_process(*self._targs)
        else:
            a = self._cargs
            L.check(_lib().kw_repeat_process(ctypes.c_void_p(a[0]), a[1], a[2], ctypes.c_void_p(a[3]), a[4],
                                             ctypes.c_void_p(a[5]), a[6], a[7], _s()), "kw_repeat_process")


class DeviceSeqTable:
    """A ``seq_bias.SeqTable`` on the device: the five arrays of ``kw_seq_bias_table`` as tensors, and the struct the
    ctypes binding passes.  ``digest`` is the host table's (plans and graphs are keyed by it)."""

    def __init__(self, table, device):
        if len(table) == 0:
            raise ValueError("an empty sequence table is no table (pass None)")
        self.digest, self.max_len = table.digest, int(table.max_len)
        self.n_seq, self.n_groups = int(table.n_seq), int(table.n_groups)
        self.tensors = [torch.from_numpy(a.copy()).to(device) for a in table.arrays()]
        c = L.SeqBiasTable()
        c.tokens, c.seq_off, c.values, c.group_off, c.group_tok = (t.data_ptr() for t in self.tensors)
        c.n_seq, c.n_groups, c.max_len = self.n_seq, self.n_groups, self.max_len
        self.c = c
        self.ref = ctypes.byref(c)


class SeqBiasPlan:
    """Pre-built ``kw_seq_bias_process`` call: one sequence table (``sequence_bias``, or ``bad_words_ids`` as -inf
    values) in place on the f32 ``scores`` [R][V], from every row's history ``ids[r][0 .. *cur_len)`` (the device
    scalar, so a captured step replays).  ``sequence_bias`` runs ahead of ``RepeatPlan``, ``bad_words_ids`` behind it,
    both ahead of ``SamplerPlan`` / ``SamplePlan``."""

    def __init__(self, scores, ids, cur_len, table: DeviceSeqTable):
        _cuda(scores, ids, cur_len)
        if scores.dim() != 2 or scores.dtype != torch.float32 or not scores.is_contiguous():
            raise ValueError("kw_seq_bias_process: scores must be a contiguous (R, V) float32 tensor")
        if (ids.dim() != 2 or ids.dtype != torch.int64 or ids.stride(1) != 1 or ids.shape[0] < scores.shape[0]
                or cur_len.dtype != torch.int32 or cur_len.numel() < 1):
            raise ValueError("kw_seq_bias_process: ids int64 [R][ids_stride], cur_len int32 [1]")
        self._keep = (scores, ids, cur_len, table)
        self._targs = (scores, ids, cur_len, table.tensors, table.max_len)
        R, V = scores.shape
        self._cargs = (scores.data_ptr(), R, V, ids.data_ptr(), ids.stride(0), cur_len.data_ptr())

    def __call__(self):
        if _BACKEND == "torch":
            _kw().seq_bias_process(*self._targs)
        else:
            a = self._cargs
            L.check(_lib().kw_seq_bias_process(ctypes.c_void_p(a[0]), a[1], a[2], ctypes.c_void_p(a[3]), a[4],
                                               ctypes.c_void_p(a[5]), self._keep[3].ref, _s()), "kw_seq_bias_process")


class BeamStepPlan:
    """Pre-built ``kw_beam_logprobs`` + ``kw_beam_select`` calls for one beam-search step.  ``repeat`` = (penalty,
    ngram): ``kw_beam_logprobs_rep`` takes ``kw_beam_logprobs``'s place (None: exactly the plain launch).  A state
    that holds ``parent_log`` (int32 [max_length][R]) and ``fin_parent`` (int32 [B][nb]) selects
    ``kw_beam_select_parents``, which also fills those two; without them the launch is ``kw_beam_select``.
    ``seq_tables`` = (sequence_bias, bad_words_ids) as ``DeviceSeqTable`` or None each: with one of them
    ``kw_beam_logprobs_proc`` is the launch (both None: exactly the launch without the argument)."""

    def __init__(self, st, logits, suppress_mask, begin_suppress, *, return_timestamps, ts_begin, no_ts_id, eos_id,
                 max_initial_ts, begin_index, max_length, fill_id, length_penalty, early_stopping, repeat=None,
                 seq_tables=None):
        """``st``: a dict of the device state tensors (see DecodeSession.generate_beam)."""
        self._rep = None if repeat is None else check_repeat(*repeat)
        self._seq = None
        if seq_tables is not None and (seq_tables[0] is not None or seq_tables[1] is not None):
            self._seq = tuple(seq_tables)
            if self._rep is None:
                self._rep = (1.0, 0)
        self._keep = (st, logits, suppress_mask, begin_suppress)
        R, V = logits.shape
        B, nb = st["fin_score"].shape
        mit = -1 if max_initial_ts is None else max_initial_ts
        es = 2 if early_stopping == "never" else int(bool(early_stopping))
        ws = st.get("lp_ws")  # split-row log-probs / top-k (kw_beam_logprobs_workspace), zero-filled once
        bp = st.get("bp")
        self._tlp = (logits, suppress_mask, begin_suppress, st["ids"], st["cur_len"], st["cand_val"], st["cand_idx"],
                     st["done"], ws, [int(bool(return_timestamps)), ts_begin, no_ts_id, eos_id, mit, begin_index, 2 * nb])
        self._tsel = (st["cand_val"], st["cand_idx"], st["ids"], bp, st["run_scores"], st["fin_seq"], st["fin_score"],
                      st["fin_len"], st["fin_flag"], st["unsat"], st["cur_len"], st["counter"], st["go"], st["done"],
                      st["item_flags"], [B, nb, V, begin_index, max_length, eos_id, fill_id, es], float(length_penalty))
        a = L.BeamLogprobsArgs()
        a.logits, a.R, a.V = logits.data_ptr(), R, V
        a.suppress_mask = suppress_mask.data_ptr()
        a.begin_suppress = begin_suppress.data_ptr() if begin_suppress is not None else None
        a.n_begin_suppress = begin_suppress.numel() if begin_suppress is not None else 0
        a.return_timestamps = int(bool(return_timestamps))
        a.ts_begin, a.no_ts_id, a.eos_id = ts_begin, no_ts_id, eos_id
        a.max_initial_ts = mit
        a.ids, a.ids_stride = st["ids"].data_ptr(), st["ids"].stride(0)
        a.cur_len = st["cur_len"].data_ptr()
        a.begin_index = begin_index
        a.k = 2 * nb
        a.cand_val, a.cand_idx, a.done = st["cand_val"].data_ptr(), st["cand_idx"].data_ptr(), st["done"].data_ptr()
        a.workspace = ws.data_ptr() if ws is not None else None
        a.ws_bytes = ws.numel() * ws.element_size() if ws is not None else 0
        b = L.BeamSelectArgs()
        b.B, b.num_beams, b.V = B, nb, V
        b.cand_val, b.cand_idx = a.cand_val, a.cand_idx
        b.ids, b.ids_stride = a.ids, a.ids_stride
        b.bp = bp.data_ptr() if bp is not None else None
        b.bp_stride = bp.stride(0) if bp is not None else 0
        b.run_scores = st["run_scores"].data_ptr()
        b.fin_seq, b.fin_stride = st["fin_seq"].data_ptr(), st["fin_seq"].shape[-1]
        b.fin_score, b.fin_len, b.fin_flag = st["fin_score"].data_ptr(), st["fin_len"].data_ptr(), st["fin_flag"].data_ptr()
        b.unsat, b.cur_len = st["unsat"].data_ptr(), a.cur_len
        b.begin_index, b.max_length, b.eos_id, b.fill_id = begin_index, max_length, eos_id, fill_id
        b.length_penalty = float(length_penalty)
        b.early_stopping = es
        b.counter, b.go, b.done = st["counter"].data_ptr(), st["go"].data_ptr(), a.done
        b.item_flags = st["item_flags"].data_ptr()
        self.a, self.b = a, b
        self._ra, self._rb = ctypes.byref(a), ctypes.byref(b)
        plog, fpar = st.get("parent_log"), st.get("fin_parent")
        if (plog is None) != (fpar is None):
            raise ValueError("beam step: parent_log and fin_parent go together")
        self._par = None
        if plog is not None:
            _cuda(plog, fpar)
            if (plog.dtype != torch.int32 or fpar.dtype != torch.int32 or not plog.is_contiguous()
                    or not fpar.is_contiguous() or plog.numel() < max_length * R or fpar.numel() < B * nb):
                raise ValueError("beam step: parent_log int32 [max_length][R], fin_parent int32 [B][num_beams]")
            self._par = (plog, fpar)

    def _select(self):
        if self._par is None:
            if _BACKEND == "torch":
                _kw().beam_select(*self._tsel)
            else:
                L.check(_lib().kw_beam_select(self._rb, _s()), "kw_beam_select")
        elif _BACKEND == "torch":
            _kw().beam_select_parents(*self._tsel, *self._par)
        else:
            L.check(_lib().kw_beam_select_parents(self._rb, _p(self._par[0]), _p(self._par[1]), _s()),
                    "kw_beam_select_parents")

    def __call__(self):
        if self._seq is not None:
            sb, bw = self._seq
            if _BACKEND == "torch":
                _kw().beam_logprobs_proc(*self._tlp, *self._rep, sb.tensors if sb else [], sb.max_len if sb else 0,
                                         bw.tensors if bw else [], bw.max_len if bw else 0)
            else:
                L.check(_lib().kw_beam_logprobs_proc(self._ra, self._rep[0], self._rep[1], sb.ref if sb else None,
                                                     bw.ref if bw else None, _s()), "kw_beam_logprobs_proc")
        elif _BACKEND == "torch":
            kw = _kw()
            if self._rep is None:
                kw.beam_logprobs(*self._tlp)
            else:
                kw.beam_logprobs_rep(*self._tlp, *self._rep)
        else:
            if self._rep is None:
                L.check(_lib().kw_beam_logprobs(self._ra, _s()), "kw_beam_logprobs")
            else:
                L.check(_lib().kw_beam_logprobs_rep(self._ra, self._rep[0], self._rep[1], _s()), "kw_beam_logprobs_rep")
        self._select()


# ---- token-level timestamps (csrc/token_ts.hip) ------------------------------------------------------------------
def _i32s(vals):
    return (ctypes.c_int32 * len(vals))(*[int(v) for v in vals])


class AlignCapturePlan:
    """Pre-built ``kw_align_capture`` call: one decode step's queries ``q`` [B][d] of one layer -> the 64-wide slices
    of ``heads`` into ``log`` [A][B][t_log][64] at slots ``slots``, position read from the device ``cur_len``."""

    def __init__(self, q, heads, slots, cur_len, begin_index, log):
        _cuda(q, cur_len, log)
        B, d = q.shape
        if log.dim() != 4 or log.shape[1] != B or log.shape[3] != 64 or log.dtype != q.dtype or not log.is_contiguous():
            raise ValueError("align capture log must be a contiguous [A][B][t_log][64] tensor of q's dtype")
        if len(heads) != len(slots) or not 0 < len(heads) <= 32:
            raise ValueError("align capture takes 1..32 heads of one layer, one log slot each")
        if any(not 0 <= h < d // 64 for h in heads) or any(not 0 <= s < log.shape[0] for s in slots):
            raise ValueError("align capture: head or log slot out of range")
        self.q, self.heads, self.slots, self.cur_len, self.begin_index, self.log = q, [int(h) for h in heads], \
            [int(s) for s in slots], cur_len, int(begin_index), log
        self.tag = "align_capture"

    def __call__(self):
        if _BACKEND == "torch":
            _kw().align_capture(self.q, self.heads, self.slots, self.cur_len, self.begin_index, self.log)
            return
        q, log = self.q, self.log
        L.check(_lib().kw_align_capture(_dt(q), _p(q), q.shape[0], q.shape[1], _i32s(self.heads), _i32s(self.slots),
                                        len(self.heads), log.shape[0], _p(self.cur_len), self.begin_index, _p(log),
                                        log.shape[2], _s()), "kw_align_capture")


def align_weights(qlog, k_cache, pairs, T, out, a0=0, layer_step=1):
    """out [A][B][T][S] f32 = softmax over s of qlog[a0 + a][b][t] . k_cache[layer * layer_step][b][head][s] for the
    ``pairs`` [(layer, head)] (<= 32 per call) and the first ``T`` logged steps."""
    _cuda(qlog, k_cache, out)
    flat = [int(v) for p in pairs for v in p]
    if _BACKEND == "torch":
        _kw().align_weights(qlog, int(a0), k_cache, int(layer_step), flat, int(T), out)
        return out
    A = len(pairs)
    B, t_log = qlog.shape[1], qlog.shape[2]
    H, S = k_cache.shape[2], k_cache.shape[3]
    if (qlog.dim() != 4 or k_cache.dim() != 5 or not qlog.is_contiguous() or not k_cache.is_contiguous()
            or k_cache.dtype != qlog.dtype or k_cache.shape[1] != B or a0 < 0 or a0 + A > qlog.shape[0]
            or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < A * B * T * S):
        raise ValueError("align_weights: qlog [A][B][t_log][64], k_cache [n][B][H][S][64], out f32 [A][B][T][S]")
    q0 = ctypes.c_void_p(qlog.data_ptr() + a0 * B * t_log * 64 * qlog.element_size())
    L.check(_lib().kw_align_weights(_dt(qlog), q0, t_log, _p(k_cache), layer_step * k_cache.stride(0),
                                    (k_cache.shape[0] + layer_step - 1) // layer_step, _i32s(flat), A, B, H, S, int(T),
                                    _p(out), _s()), "kw_align_weights")
    return out


def align_weights_rows(qlog, rows, k_cache, pairs, T, out, a0=0, layer_step=1):
    """``align_weights`` through a row table: the log holds R = B * n running rows per pair (``qlog``
    [A][R][t_log][64]) and step t of item b is the step of log row ``rows[b][t]`` (device int32 [B][T], entries in
    [0, R); the kernel clamps an entry outside): that row's query over the keys of that row's item,
    ``k_cache`` [n][B][H][S][64] at item ``rows[b][t] // n``.  ``out`` [A][B][T][S] f32."""
    _cuda(qlog, rows, k_cache, out)
    flat = [int(v) for p in pairs for v in p]
    if _BACKEND == "torch":
        _kw().align_weights_rows(qlog, int(a0), rows, k_cache, int(layer_step), flat, int(T), out)
        return out
    A = len(pairs)
    if (qlog.dim() != 4 or k_cache.dim() != 5 or not qlog.is_contiguous() or not k_cache.is_contiguous()
            or k_cache.dtype != qlog.dtype or a0 < 0 or a0 + A > qlog.shape[0] or T <= 0 or rows.dtype != torch.int32
            or not rows.is_contiguous() or rows.numel() != k_cache.shape[1] * T or out.dtype != torch.float32
            or not out.is_contiguous() or out.numel() < A * k_cache.shape[1] * T * k_cache.shape[3]):
        raise ValueError("align_weights_rows: qlog [A][R][t_log][64], rows int32 [B][T], k_cache [n][B][H][S][64], "
                         "out f32 [A][B][T][S]")
    R, t_log = qlog.shape[1], qlog.shape[2]
    B, H, S = k_cache.shape[1], k_cache.shape[2], k_cache.shape[3]
    q0 = ctypes.c_void_p(qlog.data_ptr() + a0 * R * t_log * 64 * qlog.element_size())
    L.check(_lib().kw_align_weights_rows(_dt(qlog), q0, R, t_log, _p(rows), _p(k_cache), layer_step * k_cache.stride(0),
                                         (k_cache.shape[0] + layer_step - 1) // layer_step, _i32s(flat), A, B, H, S,
                                         int(T), _p(out), _s()), "kw_align_weights_rows")
    return out


def align_reduce(weights, A, B, T, S, frames, filter_width, out, a_total=None, first=True, last=True):
    """weights [A][B][T][S] f32 -> the DTW matrix ``out`` [B][T][S] f32 (z-score over steps, median filter over the
    row's first ``frames[b]`` frames, mean over the pairs, negated); ``first`` / ``last`` chain chunks of pairs."""
    _cuda(weights, frames, out)
    a_total = A if a_total is None else a_total
    if _BACKEND == "torch":
        _kw().align_reduce(weights, A, B, T, S, frames, int(filter_width), out, int(a_total), int(first), int(last))
        return out
    if (weights.dtype != torch.float32 or out.dtype != torch.float32 or not weights.is_contiguous()
            or not out.is_contiguous() or weights.numel() < A * B * T * S or out.numel() < B * T * S
            or (frames is not None and (frames.dtype != torch.int32 or frames.numel() < B))):
        raise ValueError("align_reduce: weights [A][B][T][S] f32, out [B][T][S] f32, frames int32 [B]")
    L.check(_lib().kw_align_reduce(_p(weights), A, B, T, S, _p(frames), int(filter_width), _p(out), int(a_total),
                                   int(first), int(last), _s()), "kw_align_reduce")
    return out


def dtw_workspace_bytes(B, T, S) -> int:
    return _ws_bytes("dtw", B, T, S)


def dtw(matrix, frames=None, out=None, workspace=None):
    """matrix [B][T][S] f32 (row b: its first ``frames[b]`` columns) -> int32 [B][T]: the frame index at which the
    DTW path first reaches each step."""
    _cuda(matrix, frames, out, workspace)
    if matrix.dim() != 3 or matrix.dtype != torch.float32 or not matrix.is_contiguous():
        raise ValueError("dtw: matrix must be a contiguous [B][T][S] float32 tensor")
    B, T, S = matrix.shape
    if frames is not None and (frames.dtype != torch.int32 or frames.numel() < B):
        raise ValueError("dtw: frames must be int32 [B]")
    if out is None:
        out = torch.empty((B, T), device=matrix.device, dtype=torch.int32)
    if workspace is None:
        workspace = torch.empty((dtw_workspace_bytes(B, T, S),), device=matrix.device, dtype=torch.uint8)
    if _BACKEND == "torch":
        _kw().dtw(matrix, frames, out, workspace)
        return out
    if out.dtype != torch.int32 or not out.is_contiguous() or out.numel() < B * T:
        raise ValueError("dtw: out must be a contiguous int32 [B][T] tensor")
    L.check(_lib().kw_dtw(_p(matrix), B, T, S, _p(frames), _p(out), _p(workspace),
                          workspace.numel() * workspace.element_size(), _s()), "kw_dtw")
    return out


_KD_WS = {}  # (device index, stream handle) -> kd_loss's default workspace


def kd_loss_workspace_bytes(N: int) -> int:
    return _ws_bytes("kd_loss", N)


def kd_loss(teacher, student, labels, temperature, grad=None, row_kl=None, loss=None, workspace=None):
    """``kw_kd_loss``: the temperature KL of run_distillation.py:614-622,652-657 on logits [N][V] (row stride >= V,
    unit inner stride; rows need no alignment).  teacher f32, student f32 or bf16, labels int64 [N] (negative =
    ignored row).  Returns (loss f32 [1], row_kl f32 [N]); ``grad`` ([N][V], the student's dtype), when given, takes
    d loss / d student = T (q - p) / n_valid.  Nothing synchronises with the host."""
    _cuda(teacher, student, labels, grad, row_kl, loss, workspace)
    if teacher.dim() != 2 or teacher.dtype != torch.float32 or teacher.stride(1) != 1:
        raise ValueError("kw_kd_loss: teacher must be an (N, V) float32 tensor with unit inner stride")
    N, V = teacher.shape
    if student.dim() != 2 or tuple(student.shape) != (N, V) or student.stride(1) != 1:
        raise ValueError("kw_kd_loss: student must be an (N, V) tensor like teacher, with unit inner stride")
    sdt = _dt(student)
    if labels.dim() != 1 or labels.shape[0] != N or labels.dtype != torch.int64 or not labels.is_contiguous():
        raise ValueError("kw_kd_loss: labels must be a contiguous int64 [N] tensor")
    if grad is not None and (grad.dim() != 2 or tuple(grad.shape) != (N, V) or grad.stride(1) != 1
                             or grad.dtype != student.dtype):
        raise ValueError("kw_kd_loss: grad must be an (N, V) tensor of the student's dtype with unit inner stride")
    if N < 1 or V < 1:
        raise ValueError("kw_kd_loss: 1 <= N, V < 2^31 and every row stride >= V")
    dev = teacher.device
    if row_kl is None:
        row_kl = torch.empty((N,), device=dev, dtype=torch.float32)
    if loss is None:
        loss = torch.empty((1,), device=dev, dtype=torch.float32)
    if (row_kl.dtype != torch.float32 or not row_kl.is_contiguous() or row_kl.numel() != N
            or loss.dtype != torch.float32 or loss.numel() != 1):
        raise ValueError("kw_kd_loss: row_kl float32 [N], loss float32 [1]")
    if workspace is None:
        # zero-filled once per (device, stream) and kept: calls leave it zeroed, and calls on one stream are ordered
        key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
        workspace = _KD_WS.get(key)
        if workspace is None or workspace.numel() < kd_loss_workspace_bytes(N):
            workspace = _KD_WS[key] = torch.zeros((kd_loss_workspace_bytes(N),), device=dev, dtype=torch.uint8)
    if _BACKEND == "torch":
        _kw().kd_loss(teacher, student, labels, float(temperature), row_kl, loss, grad, workspace)
        return loss, row_kl
    ld = (lambda t: V if N == 1 else t.stride(0))  # (a one-row tensor's stride(0) is arbitrary)
    a = L.KdLossArgs(_p(teacher), ld(teacher), _p(student), ld(student), sdt, _p(labels), N, V, float(temperature),
                     _p(row_kl), _p(loss), _p(grad), 0 if grad is None else ld(grad), _p(workspace),
                     workspace.numel() * workspace.element_size())
    L.check(_lib().kw_kd_loss(ctypes.byref(a), _s()), "kw_kd_loss")
    return loss, row_kl
