"""Speculative (assisted) greedy decoding for one row: a small assistant decoder drafts, the main decoder verifies.

``SpecDecodeSession`` pairs a main ``DecodeSession(B=1)`` with an assistant ``DecodeSession(B=1)`` of a second engine.
Both decode ONE token history: the assistant session's ``ids`` is the main session's buffer.  One round is one captured
hipGraph:

  * draft   K + 1 replays of the assistant's ordinary greedy step.  The first K write the drafts ids[L, L + K); the
            last one only ingests draft K, so that after a full accept the assistant's cache is complete (its own
            output, ids[L + K], is overwritten by the accept step).  The assistant runs the main model's Whisper
            processors, without SuppressTokensAtBegin and with a ``max_length`` it cannot reach.
  * verify  the main decoder's forward over the K + 1 newest positions [L - 1, L + K) (``_step_plans(K + 1)`` reading
            ``verify_len`` = L + K instead of the session's ``cur_len``), the LM head on all K + 1 rows.
  * accept  ``kw_spec_accept`` (csrc/spec.hip): every position's greedy token with the drafts in place, the longest
            agreeing prefix, the correction or bonus token, and the device state of both decoders for the next round.

The host replays rounds and reads (unfinished rows, length) one round behind the device.  A round touches positions up
to L + K, and a replay issued behind a row that has just finished drafts once more from the final length, so rounds
are issued only while the host's upper bound Lb on L satisfies Lb + K + 1 <= max_length and Lb + 2 K + 1 <= T_MAX;
the rest is decoded by the main session's plain one-token step graph.  The output is the main model's own greedy
output: a draft only ever survives where the main model's processed arg-max agrees with it.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .decode import T_MAX, DecodeSession, _reference_length, capture_graph


def _device_index(dev) -> int:
    dev = torch.device(dev)
    return torch.cuda.current_device() if dev.index is None else dev.index


class SpecDecodeSession:
    def __init__(self, main_eng, asst_eng):
        if main_eng.shape.vocab_size != asst_eng.shape.vocab_size:
            raise ValueError("the assistant model's vocabulary differs from the main model's")
        if getattr(main_eng, "cross_kv_fp8", False) or getattr(asst_eng, "cross_kv_fp8", False):
            raise NotImplementedError("assisted generate with cross_kv_dtype='fp8_e4m3'")
        if _device_index(main_eng.device) != _device_index(asst_eng.device):
            # one ids buffer, and the accept launch writes the assistant's device scalars on the main engine's stream
            raise ValueError(f"the assistant model must be on the main model's device ({main_eng.device}), not on "
                             f"{asst_eng.device}")
        self.main: DecodeSession = main_eng.new_session(1)
        self.asst: DecodeSession = asst_eng.new_session(1)
        # These two sessions never evict a buffer set: the captured round graphs kept in ``_cfg`` hold the addresses of
        # the verify forward's K + 1-position buffers, and DecodeSession's eviction of long prefill lengths (q > LONG_Q,
        # i.e. K >= 8) would free them under a graph still cached here.  There is no long prompt to bound instead
        # (prompts are refused with an assistant): the sets are a few tokens' prompt lengths and at most 31 values of
        # K + 1 <= 32 rows each.
        self.main._long_q = self.asst._long_q = None
        self.asst.ids = self.main.ids  # one token history (before any plan of the assistant session is built)
        dev = main_eng.device
        self.verify_len = torch.zeros((1,), device=dev, dtype=torch.int32)
        self.stats = torch.zeros((3,), device=dev, dtype=torch.int32)  # rounds, drafted, accepted
        self._vlogits = {}  # K -> f32 [K + 1][V]
        self._ws = {}       # K -> kw_spec_accept workspace (zeroed once; launches leave it zeroed)
        self._cfg = {}
        self._pinned = None
        self.last_rounds = self.last_steps = 0

    def set_encoder_output(self, enc_main: torch.Tensor, enc_asst: torch.Tensor) -> None:
        self.main.set_encoder_output(enc_main)
        self.asst.set_encoder_output(enc_asst)

    def _config(self, K, P, gen, max_length, return_timestamps):
        key = (K, P, max_length, bool(return_timestamps), tuple(gen.suppress_tokens or ()), gen.timestamp_begin,
               gen.no_timestamps_token_id, gen.eos_token_id, gen.pad_token_id, gen.max_initial_timestamp_index,
               self.main.eng.prefill_streams)
        cfg = self._cfg.get(key)
        if cfg is not None:
            return cfg
        m, a = self.main, self.asst
        dev, V = m.eng.device, m.eng.shape.vocab_size
        sup = torch.zeros((V,), dtype=torch.uint8)
        if gen.suppress_tokens:
            sup[torch.tensor(gen.suppress_tokens)] = 1
        sup = sup.to(dev)
        pcfg = dict(return_timestamps=return_timestamps, ts_begin=gen.timestamp_begin,
                    no_ts_id=gen.no_timestamps_token_id, eos_id=gen.eos_token_id, pad_id=gen.pad_token_id,
                    max_initial_ts=gen.max_initial_timestamp_index, begin_index=P)
        # SuppressTokensAtBegin is dropped with an assistant (TF generation_whisper.py:718-720)
        main_sampler = ops.SamplerPlan(m.logits, sup, None, m.ids, m.cur_len, m.unfinished, m.counter, m.n_unfinished,
                                       workspace=m.samp_ws, max_length=max_length, **pcfg)
        asst_sampler = ops.SamplerPlan(a.logits, sup, None, a.ids, a.cur_len, a.unfinished, a.counter, a.n_unfinished,
                                       workspace=a.samp_ws, max_length=T_MAX + 1, **pcfg)
        if K not in self._vlogits:
            self._vlogits[K] = torch.empty((K + 1, V), device=dev, dtype=torch.float32)
            self._ws[K] = torch.zeros(((ops.spec_accept_workspace_bytes(K) + 3) // 4,), device=dev, dtype=torch.float32)
        accept = ops.SpecAcceptPlan(self._vlogits[K], sup, None, m.ids, m.cur_len, m.unfinished, m.n_unfinished, K=K,
                                    max_length=max_length, workspace=self._ws[K], asst_cur_len=a.cur_len,
                                    asst_unfinished=a.unfinished, verify_len=self.verify_len, stats=self.stats, **pcfg)
        cfg = dict(main_sampler=main_sampler, asst_sampler=asst_sampler, accept=accept, P=P)
        if len(self._cfg) >= 4:  # bound the cache (each entry holds graphs)
            self._cfg.pop(next(iter(self._cfg)))
        self._cfg[key] = cfg
        return cfg

    def _poll2(self, events, rep, lag):
        """Queue copies of (unfinished rows, length) behind the replay just issued and read the pair queued ``lag``
        replays ago: (n_unfinished, cur_len), or None while fewer than ``lag`` replays are behind."""
        if self._pinned is None:
            self._pinned = torch.zeros((8, 2), dtype=torch.int32).pin_memory()
        slot = rep % (lag + 1)
        self._pinned[slot] = -1
        self._pinned[slot, 0:1].copy_(self.main.n_unfinished, non_blocking=True)
        self._pinned[slot, 1:2].copy_(self.main.cur_len, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        events.append((ev, slot))
        if len(events) > lag:
            e0, s0 = events.pop(0)
            e0.synchronize()
            return int(self._pinned[s0, 0]), int(self._pinned[s0, 1])
        return None

    def generate(self, prompt: torch.Tensor, gen, *, K: int, max_length: int, return_timestamps: bool,
                 check_every: int = 4) -> np.ndarray:
        """Assisted greedy decoding of one row; host int64 ids (1, L) including the prompt, as
        ``DecodeSession.generate`` returns them for the main model with ``begin_suppress_tokens=None``."""
        m, a = self.main, self.asst
        K = int(K)
        if not 1 <= K <= ops.SPEC_K_MAX:
            raise ValueError(f"num_assistant_tokens must be in [1, {ops.SPEC_K_MAX}]")
        if prompt.shape[0] != 1:
            raise ValueError("assisted generate is only supported for batch_size = 1")
        P = prompt.shape[1]
        if P + 1 > T_MAX + 1 or max_length > T_MAX:
            raise ValueError(f"max_length {max_length} exceeds max_target_positions {T_MAX}")
        dev = m.eng.device
        cfg = self._config(K, P, gen, max_length, return_timestamps)
        m.ids.zero_()
        m.ids[:, :P].copy_(prompt.to(dev))
        for s in (m, a):
            s.cur_len.fill_(P)
            s.unfinished.fill_(1)
            s.counter.zero_()
            s.n_unfinished.fill_(1)
        self.stats.zero_()
        main_sampler, asst_sampler, accept = cfg["main_sampler"], cfg["asst_sampler"], cfg["accept"]

        # ---- prefill of both decoders; the first token is the main model's ----
        def prefill():
            a._run(a._step_plans(P))
            m._run_prefill(P, m.eng.prefill_streams)
            main_sampler()
            a.cur_len.fill_(P + 1)
            self.verify_len.fill_(P + 1 + K)

        def graph_of(name, fn):
            if name not in cfg:  # (capture only records: the state the launches consume is untouched until the replay)
                cfg[name] = capture_graph(fn, dev)
            return cfg[name]

        graph_of("prefill_graph", prefill).replay()

        fused = max_length <= 256  # every step's position < 256 (kw_dec_qkv_self's key range)
        a_step = a._step_plans(1, fused=fused)
        m_step = m._step_plans(1, fused=fused)
        verify = m._step_plans(K + 1, all_rows=self._vlogits[K])

        def one_round():
            for _ in range(K + 1):
                a._run(a_step)
                asst_sampler()
            m._run(verify, cur_len=self.verify_len)
            accept()

        def one_step():
            m._run(m_step)
            main_sampler()

        stream = torch.cuda.current_stream(dev)
        rounds = steps = 0
        lag = 1  # a round is many launches long: one round in flight behind the host hides the poll
        L_now, unfinished = P + 1, True
        while True:
            # ---- rounds, while the host's bound on the length leaves room for a whole one (module docstring) ----
            Lb, events, rep = L_now, [], 0
            while Lb + K + 1 <= max_length and Lb + 2 * K + 1 <= T_MAX:
                graph_of("round_graph", one_round).replay()
                rounds += 1
                Lb += K + 1
                seen = self._poll2(events, rep, lag)
                rep += 1
                if seen is not None:
                    if seen[0] == 0:
                        break
                    Lb = min(Lb, seen[1] + lag * (K + 1))
            stream.synchronize()
            L_now, unfinished = int(m.cur_len.item()), int(m.n_unfinished.item()) != 0
            if not unfinished or L_now >= max_length:
                break
            if L_now + K + 1 <= max_length and L_now + 2 * K + 1 <= T_MAX:
                continue  # the bound was loose: room for more rounds
            # ---- the plain-step tail ----
            n_steps = max_length - L_now
            pinned = m._pinned_slots(check_every + 1)
            events, done = [], 0
            while done < n_steps:
                graph_of("step_graph", one_step).replay()
                done += 1
                if m._poll(pinned, events, done - 1, check_every, m.n_unfinished):
                    break
            steps += done
            stream.synchronize()
            L_now = int(m.cur_len.item())
            break
        self.last_rounds, self.last_steps = rounds, steps
        m.check_handoffs()
        a.check_handoffs()
        self.last_stats = dict(zip(("rounds", "drafted", "accepted"), (int(x) for x in self.stats.cpu().tolist())))
        ids = m.ids[:, :L_now].cpu().numpy()
        return _reference_length(ids, P, gen.eos_token_id, max_length)
