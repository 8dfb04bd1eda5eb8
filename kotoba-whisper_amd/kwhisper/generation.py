"""HF-compatible drop-in: ``WhisperForConditionalGeneration.generate()`` on the MI355X engine.

The object returned by ``from_pretrained``/``from_state_dict`` is what the reference passes as
``model`` at run_pseudo_labelling.py:338 (and v3 :313-318) and what the ASR pipeline's ``_forward``
calls at TF/pipelines/automatic_speech_recognition.py:529.  It keeps HF's call signature,
argument meaning, errors and token output (transformers 5.15.0,
TF/models/whisper/generation_whisper.py:383-968):

  * prompt ``[sot, lang, task(, notimestamps)]``                     :1455-1608
  * language detection when ``language`` is None (multilingual)      :1620-1674
  * processors Suppress -> SuppressAtBegin -> TimeStamp (on device)  :1774-1812
  * the seek loop with the cumulative ``max_length`` growth          :785-903, :1920-1946
  * strip prompt / pad-count quirk / strip EOS                       :1042-1086
  * segments and right padding with ``pad_token_id``                 :1977-2074, :126-237
  * ``return_dict_in_generate`` (no timestamps): sequences incl. prompt  :916-934
  * ``num_beams`` > 1: GenerationMixin._beam_search on device (TF/generation/utils.py:3208-3527)
  * ``return_token_timestamps``: the alignment heads' cross-attention weights, their normalisation and the
    dynamic time warping on device (csrc/token_ts.hip)                :241-381, :1146-1157, :1685-1700
    -- with ``num_beams`` > 1 too: every running row's queries are logged, the beam step records its parents
    (kw_beam_select_parents), the host backtraces the returned hypotheses to ``beam_indices`` and the weights are read
    through that table (kw_align_weights_rows); a row shorter than the pass's longest reads running row 0 of the
    pass for its remaining steps, as the reference does                :265-301
    (not together with the fallback, prompts or the fp8 cross cache; asked of the engine, ``beam_token_ts``)
  * the decoding fallback -- ``temperature`` (a float or a schedule), ``compression_ratio_threshold``,
    ``logprob_threshold``, ``no_speech_threshold``: per seek pass the attempt loop of ``generate_with_fallback``, every
    row's ``_need_fallback`` decision, the no-speech skip; tokens drawn and log-probabilities accumulated on device
    (kw_sample_step, csrc/sampling.hip)                               :970-1116, :1243-1287, :876-881, :1949-1974
  * ``prompt_ids`` / ``prompt_condition_type`` / ``condition_on_prev_tokens``: per seek pass the decoder input of
    ``_prepare_decoder_input_ids`` -- the previous text behind ``<|startofprev|>``, left-padded to the pass's longest
    row -- built on the host (``build_pass_input``); the pads are masked in the decoder self-attention by a per-row
    first key (kw_self_attn_step_masked), positions stay the plain arange     :1853-1918, :126-235, :1119-1126, :905-915
  * ``repetition_penalty`` / ``no_repeat_ngram_size`` (from the call, else the generation config):
    RepetitionPenaltyLogitsProcessor -> NoRepeatNGramLogitsProcessor ahead of the Whisper processors, on device in
    every step of every pass and every fallback attempt -- on the raw logits for the greedy and sampled tails
    (kw_repeat_process, csrc/repeat.hip), on the log-probs for beams (kw_beam_logprobs_rep, csrc/beam.hip)
                                              TF/generation/utils.py:1174-1183, TF/generation/logits_process.py:406-413, 1121-1139
    ``generate_multitask``, ``pseudo_label*`` and ``ASRPipeline(generate_kwargs=...)`` forward their keywords to
    ``generate`` unchanged, so the two reach it from there as well.
  * ``sequence_bias`` / ``bad_words_ids`` (from the call, else the generation config): SequenceBiasLogitsProcessor
    immediately ahead of that pair, NoBadWordsLogitsProcessor immediately behind it, both ahead of the Whisper
    processors, on device in every step of every pass and every fallback attempt -- kw_seq_bias_process on the raw
    logits (csrc/seqbias.hip), kw_beam_logprobs_proc on the log-probs for beams (csrc/beam.hip); the host flattens
    each processor into a table once (kwhisper/seq_bias.py)
                                              TF/generation/utils.py:1154-1155, 1207-1213, TF/generation/logits_process.py:1288-1319, 1450-1467
  * ``assistant_model`` / ``num_assistant_tokens``: assisted (speculative) decoding at batch size 1 -- per seek pass
    the assistant (another ``KWhisperForConditionalGeneration``) encodes the features with its own encoder and drafts
    K tokens with its greedy step, this model checks them in one K + 1-position forward and ``kw_spec_accept``
    (csrc/spec.hip) keeps the longest agreeing prefix plus the correction or bonus token (kwhisper/spec.py, one hipGraph
    per round).  The tokens are this model's own greedy tokens with ``begin_suppress_tokens=None``, which the
    reference drops with an assistant (:718-720); ``stats["assisted"]`` = rounds, drafted, accepted.
                                              TF/generation/utils.py ``_assisted_decoding``, TF/generation/candidate_generator.py

Deliberate differences of assisted generate from transformers 5.15.0:
  * K is constant: from the call, else the assistant's ``generation_config.num_assistant_tokens``, else 5.  The
    reference's default schedule changes K with the acceptance, which changes speed only, never tokens;
  * the tokens are held to this engine's greedy ``generate()``, not to the reference's assisted output: on the tiny
    synthetic fixtures (CPU) that path equals the reference's own greedy output only on some ``return_timestamps=False``
    rows, raises ``IndexError`` past position 448 on others, and with ``return_timestamps=True`` returns sequences of
    hundreds to thousands of tokens.

Deliberate differences of the fallback from transformers 5.15.0:
  * ``no_speech_threshold`` without ``logprob_threshold`` raises ``ValueError`` (the reference dies on an unbound local);
  * ``temperature=None`` together with a threshold is treated as 0.0 (the reference raises ``TypeError``);
  * every decision is made with the row's own numbers.  The reference indexes ``should_skip`` and ``no_speech_prob`` by
    the row's position in the *current* attempt's batch, so once rows have left the fallback set it reads and writes
    other rows' entries; the two agree while no row is skipped after the first attempt;
  * a row's tokens are counted up to and including its first EOS; the reference counts pad tokens anywhere in the row
    when it strips the padding (:1063-1071), which differs only for a padded row that also sampled the pad token;
  * sampled tokens come from the engine's own counter-based generator (``manual_seed``), so they are distributed as
    the reference's (softmax(s / T), multinomial) but are not the same draws as torch's;
  * ``do_condition_on_prev_tokens`` after a fallback attempt is kept per audio; the reference writes it at the row's
    position in the pass's batch (:1091) and reads it by the audio's index (:1884), which differ once an audio has left
    the batch.
"""
from __future__ import annotations

import copy
import itertools
import math
import os
import zlib
from dataclasses import dataclass

import numpy as np
import torch

from .config import PRESETS, GenerationConstants, WhisperShape, generation_constants, language_to_id
from . import seq_bias
from .engine import WhisperEngine

_SUPPORTED = {
    "generation_config", "logits_processor", "stopping_criteria", "return_timestamps", "task", "language",
    "is_multilingual", "attention_mask", "max_length", "max_new_tokens", "num_beams", "return_dict_in_generate",
    "return_segments", "encoder_outputs", "prompt_ids", "temperature", "do_sample", "condition_on_prev_tokens",
    "compression_ratio_threshold", "logprob_threshold", "no_speech_threshold", "return_token_timestamps",
    "output_scores", "output_logits", "time_precision", "time_precision_features", "num_segment_frames",
    "synced_gpus", "force_unique_generate_call", "prefix_allowed_tokens_fn", "prompt_condition_type",
    "monitor_progress", "use_cache", "num_return_sequences", "length_penalty", "early_stopping",
    "repetition_penalty", "no_repeat_ngram_size", "assistant_model", "num_assistant_tokens",
    "sequence_bias", "bad_words_ids",
}


@dataclass
class ModelConfig:
    """The ``model.config`` fields callers read (run_pseudo_labelling.py:233,295)."""

    shape: WhisperShape

    def __getattr__(self, k):
        return getattr(self.shape, k)


class EncoderOutput:
    def __init__(self, h):
        self.last_hidden_state = h

    def __getitem__(self, i):
        if i == 0:
            return self.last_hidden_state
        raise IndexError(i)


def shift_tokens_right(input_ids: torch.Tensor, pad_token_id: int, decoder_start_token_id: int) -> torch.Tensor:
    """Labels -> decoder input ids (TF modeling_whisper.py ``shift_tokens_right``): one step to the right behind
    ``decoder_start_token_id``, every -100 replaced by ``pad_token_id``."""
    if pad_token_id is None:
        raise ValueError("self.model.config.pad_token_id has to be defined.")
    shifted = input_ids.new_zeros(input_ids.shape)
    shifted[:, 1:] = input_ids[:, :-1]
    shifted[:, 0] = decoder_start_token_id
    shifted.masked_fill_(shifted == -100, pad_token_id)
    return shifted


class ForwardOutput:
    """What ``forward()`` returns, read as HF's ``Seq2SeqLMOutput``: attributes, string keys, and the tuple of the
    fields that are not None -- ``out[0]`` is the loss when there were labels, otherwise the logits."""

    def __init__(self, logits, encoder_last_hidden_state, labels=None):
        self.logits = logits
        self.encoder_last_hidden_state = encoder_last_hidden_state
        self._labels = labels
        self._loss = None

    @property
    def loss(self):
        """HF's ``CrossEntropyLoss()(logits.view(-1, V), labels.reshape(-1))``: the mean of -log softmax(logits)[label]
        over the positions whose label is not -100, by torch ops on the f32 logits (no copy of them: a log-sum-exp
        and a gather); None without labels."""
        if self._labels is None:
            return None
        if self._loss is None:
            with torch.no_grad():
                valid = self._labels != -100
                picked = self.logits.gather(-1, self._labels.clamp(min=0).unsqueeze(-1)).squeeze(-1)
                nll = (torch.logsumexp(self.logits, -1) - picked) * valid
                self._loss = nll.sum() / valid.sum()
        return self._loss

    def keys(self):
        return [k for k in ("loss", "logits", "encoder_last_hidden_state") if getattr(self, k) is not None]

    def to_tuple(self):
        return tuple(getattr(self, k) for k in self.keys())

    def __getitem__(self, i):
        return getattr(self, i) if isinstance(i, str) else self.to_tuple()[i]

    def __iter__(self):  # (a ModelOutput is a dict: iterating gives its keys)
        return iter(self.keys())

    def __len__(self):
        return len(self.keys())


class _Encoder:
    """``model.get_encoder()``: returns (B, 1500, d) last_hidden_state (modeling_whisper.py:592-646)."""

    def __init__(self, eng):
        self.eng = eng

    def __call__(self, input_features, **kw):
        B = input_features.shape[0]
        h = self.eng.encode(input_features)
        return EncoderOutput(h.view(B, self.eng.shape.max_source_positions, self.eng.shape.d_model))


class KWhisperForConditionalGeneration:
    main_input_name = "input_features"

    def __init__(self, engine: WhisperEngine):
        self.engine = engine
        self.config = ModelConfig(engine.shape)
        self.generation_config = engine.generation_config
        self._sessions = {}
        self._spec_sessions = {}  # id(assistant engine) -> the paired SpecDecodeSession
        self._fwd_sessions = {}  # batch size -> forward()'s own DecodeSession
        # validation: "wide" / "chunk" forces the bf16 engine's many-row plan of forward() (None: by the row count)
        self.forward_plan = None
        self.stats = {}
        # True: generate() also keeps every seek pass's decoded ids in stats["pass_ids"] (validation: a fixture of the
        # engine's own multi-pass trajectory, tools/dump_hipmel.py)
        self.record_pass_ids = False
        # True: generate(return_token_timestamps=True) also keeps every pass's alignment results (frame indices, the
        # DTW matrix, the raw weights) in stats["alignment"] (validation)
        self.record_alignment = False
        self._memo = None  # generate_multitask's per-batch encoder memo
        self._memo_count = 0
        # sampling: kw_sample_step's Philox key is the seed; its attempt word is (lane << 24) | a counter that advances on
        # every sampled decode, so attempts, passes and lane() handles all draw from distinct streams
        self._seed, self._attempts, self._lane = 0, 0, 0
        self._lane_ids = itertools.count(1)  # shared by every handle lane() makes from this one
        self._sot_logits = None  # detect_language's raw logits at <|startoftranscript|>, for the no-speech probability

    # ---- nn.Module-ish surface used by callers ---------------------------------------------------
    @property
    def device(self):
        return self.engine.device

    @property
    def dtype(self):
        return self.engine.dtype

    def eval(self):
        return self

    def to(self, *a, **k):
        return self

    def get_encoder(self):
        return _Encoder(self.engine)

    def lane(self) -> "KWhisperForConditionalGeneration":
        """An independent handle on the same weights (WhisperEngine.lane(): own activation buffers, streams and decode
        sessions) for running another batch at the same time from another host thread."""
        other = type(self)(self.engine.lane())
        other.generation_config = copy.deepcopy(self.generation_config)
        other._seed, other._lane_ids = self._seed, self._lane_ids
        other._lane = next(self._lane_ids)
        return other

    def manual_seed(self, seed: int) -> "KWhisperForConditionalGeneration":
        """Seed the sampler of the temperature fallback (default 0) and restart its attempt counter: the same calls
        after the same ``manual_seed`` draw the same tokens."""
        self._seed, self._attempts = int(seed), 0
        return self

    @classmethod
    def from_state_dict(cls, shape, state_dict, *, dtype=torch.bfloat16, device="cuda", generation_config=None,
                        cross_kv_dtype=None):
        """``cross_kv_dtype``: None / "bf16" (the default engine) or "fp8_e4m3" (WhisperEngine: the cross-attention K/V
        cache as e4m3 codes with per-channel scales; bf16 engine, greedy decoding only)."""
        shape = PRESETS[shape] if isinstance(shape, str) else shape
        return cls(WhisperEngine(shape, state_dict, dtype=dtype, device=device, generation_config=generation_config,
                                 cross_kv_dtype=cross_kv_dtype))

    @classmethod
    def from_pretrained(cls, path_or_name, *, torch_dtype=torch.bfloat16, device="cuda", cross_kv_dtype=None, **kw):
        """Load a local HF checkpoint directory (config.json + *.safetensors).  No network access."""
        import json

        from safetensors.numpy import load_file

        if not os.path.isdir(path_or_name):
            raise OSError(f"{path_or_name} is not a local checkpoint directory (no hub access in this build)")
        cfg = json.load(open(os.path.join(path_or_name, "config.json")))
        shape = WhisperShape(
            name=cfg.get("_name_or_path", path_or_name), vocab_size=cfg["vocab_size"], num_mel_bins=cfg["num_mel_bins"],
            d_model=cfg["d_model"], encoder_layers=cfg["encoder_layers"],
            encoder_attention_heads=cfg["encoder_attention_heads"], encoder_ffn_dim=cfg["encoder_ffn_dim"],
            decoder_layers=cfg["decoder_layers"], decoder_attention_heads=cfg["decoder_attention_heads"],
            decoder_ffn_dim=cfg["decoder_ffn_dim"], max_source_positions=cfg.get("max_source_positions", 1500),
            max_target_positions=cfg.get("max_target_positions", 448),
            median_filter_width=cfg.get("median_filter_width", 7),
            decoder_start_token_id=cfg.get("decoder_start_token_id", 50258), pad_token_id=cfg.get("pad_token_id", 50256),
            eos_token_id=cfg.get("eos_token_id", 50257), bos_token_id=cfg.get("bos_token_id", 50257))
        sd = {}
        for f in sorted(os.listdir(path_or_name)):
            if f.endswith(".safetensors"):
                sd.update(load_file(os.path.join(path_or_name, f)))
        gen = generation_constants(shape)
        gpath = os.path.join(path_or_name, "generation_config.json")
        if os.path.exists(gpath):
            gj = json.load(open(gpath))
            for k, v in gj.items():
                if hasattr(gen, k):
                    setattr(gen, k, v)
        return cls.from_state_dict(shape, sd, dtype=torch_dtype, device=device, generation_config=gen,
                                   cross_kv_dtype=cross_kv_dtype)

    # ---- generate ---------------------------------------------------------------------------------
    def _session(self, B, beams=1):
        key = (B, beams)
        if key not in self._sessions:
            self._sessions[key] = self.engine.new_session(B, beams=beams)
        return self._sessions[key]

    def _spec_session(self, assistant):
        """The paired session of assisted generate (kwhisper/spec.py) with ``assistant``'s engine, kept per assistant."""
        from .spec import SpecDecodeSession

        key = id(assistant.engine)
        if key not in self._spec_sessions:
            self._spec_sessions[key] = (SpecDecodeSession(self.engine, assistant.engine), assistant.engine)
        return self._spec_sessions[key][0]

    # ---- forward (the teacher's no-grad pass of a distillation step) -------------------------------
    def forward(self, input_features=None, attention_mask=None, decoder_input_ids=None, encoder_outputs=None,
                labels=None, **unsupported):
        """``WhisperForConditionalGeneration.forward`` (TF modeling_whisper.py, transformers 5.15.0) for inference:
        what kotoba-whisper's ``train_step`` asks of its frozen teacher, ``teacher_model(**batch)`` or
        ``teacher_model(encoder_outputs=..., labels=...)`` (run_distillation.py:641-657).

        ``decoder_input_ids`` is used as given; without it the labels are shifted right behind
        ``decoder_start_token_id`` with -100 replaced by ``pad_token_id`` (``shift_tokens_right``).  ``attention_mask``
        is accepted and ignored (the reference's encoder reads it for SpecAugment only).  ``encoder_outputs``: what
        ``generate(encoder_outputs=)`` takes -- a tensor, a tuple or an object with ``last_hidden_state``.  Any
        other keyword that is not None raises ``NotImplementedError``.

        Returns a ``ForwardOutput``: ``.logits`` f32 [B, T, V] on the device -- always f32, where the reference's
        bf16 model returns bf16 -- ``.encoder_last_hidden_state`` and ``.loss`` (HF's cross-entropy over ``labels``,
        computed on first access; None without labels).  Never builds an autograd graph."""
        for k, v in unsupported.items():
            if v is not None:
                raise NotImplementedError(f"`{k}` is not supported by the MI355X engine's forward()")
        s = self.engine.shape
        if labels is not None:
            if labels.shape[1] > s.max_target_positions:
                raise ValueError(f"Labels' sequence length {labels.shape[1]} cannot exceed the maximum allowed length "
                                 f"of {s.max_target_positions} tokens.")
            if decoder_input_ids is None:
                decoder_input_ids = shift_tokens_right(labels, s.pad_token_id, s.decoder_start_token_id)
        if decoder_input_ids is None:  # (WhisperDecoder.forward's check, with no decoder_inputs_embeds to offer)
            raise ValueError("You cannot specify both decoder_input_ids and decoder_inputs_embeds at the same time")
        if input_features is None and encoder_outputs is None:
            raise ValueError("Make sure to provide either `input_features` or `encoder_outputs` to `forward`.")
        if decoder_input_ids.dim() != 2 or not 1 <= decoder_input_ids.shape[1] <= s.max_target_positions:
            raise ValueError(f"`decoder_input_ids` must be (batch, 1 .. {s.max_target_positions})")
        eng = self.engine
        if getattr(eng, "cross_kv_fp8", False):
            raise NotImplementedError("forward() is not supported with cross_kv_dtype='fp8_e4m3' (there is no many-row "
                                      "fp8 cross-attention kernel); use the bf16 cache")
        with torch.no_grad():
            ids = decoder_input_ids.to(device=eng.device, dtype=torch.int64)
            B = ids.shape[0]
            if bool(((ids < 0) | (ids >= s.vocab_size)).any()):  # (the embedding gathers by id: never out of the table)
                raise IndexError(f"`decoder_input_ids` must lie in [0, {s.vocab_size})")
            if encoder_outputs is None:
                if input_features.shape[0] != B:
                    raise ValueError("`input_features` and `decoder_input_ids` must share the batch size")
                enc = eng.encode(input_features.to(device=eng.device, dtype=torch.float32))
            else:  # (given encoder outputs are used and the encoder skipped, with or without input_features, as HF does)
                eh = encoder_outputs.last_hidden_state if hasattr(encoder_outputs, "last_hidden_state") else \
                    encoder_outputs[0] if isinstance(encoder_outputs, (tuple, list)) else encoder_outputs
                if eh.dim() != 3 or tuple(eh.shape) != (B, s.max_source_positions, s.d_model):
                    raise ValueError(f"`encoder_outputs` must be ({B}, {s.max_source_positions}, {s.d_model})")
                enc = eh.to(eng.device, eng.dtype).reshape(B * s.max_source_positions, s.d_model).contiguous()
            sess = self._forward_session(B)
            sess.set_encoder_output(enc)
            logits = sess.forward_all(ids, plan=self.forward_plan)
            # (the encoder's output buffer is the engine's: the caller gets a tensor of its own)
            enc_out = enc.view(B, s.max_source_positions, s.d_model).clone()
        return ForwardOutput(logits, enc_out, None if labels is None else labels.to(eng.device))

    __call__ = forward

    FORWARD_SESSIONS = 2  # batch sizes whose forward() session stays alive (an epoch's batch size and its last batch)

    def _forward_session(self, B):
        """forward()'s decode session of batch size B: its own, so that nothing generate() reads (ids, caches, cross
        K/V, step buffers, captured graphs) is touched by a forward in between.  The ``FORWARD_SESSIONS`` most recently
        used batch sizes keep theirs (about 10 GB at large-v3, B = 32); an older one is released."""
        fs = self._fwd_sessions
        sess = fs.pop(B, None)
        if sess is None:
            while len(fs) >= self.FORWARD_SESSIONS:
                del fs[next(iter(fs))]  # the least recently used (dicts keep insertion order)
            sess = self.engine.new_session(B)
        fs[B] = sess
        return sess

    def generate(self, input_features=None, generation_config=None, logits_processor=None, stopping_criteria=None,
                 return_timestamps=None, task=None, language=None, is_multilingual=None, attention_mask=None,
                 return_dict_in_generate=None, return_segments=False, **kwargs):
        unknown = [k for k in kwargs if k not in _SUPPORTED]
        if unknown:
            raise ValueError(
                f"The following `model_kwargs` are not used by the model: {unknown} (note: typos in the generate "
                "arguments will also show up in this list)"
            )
        if logits_processor or stopping_criteria:
            raise NotImplementedError("custom logits_processor / stopping_criteria are not supported on device")
        for k in ("prefix_allowed_tokens_fn", "output_scores"):
            if kwargs.get(k) is not None and kwargs.get(k) is not False:
                raise NotImplementedError(f"`{k}` is not supported by the MI355X engine yet")
        if kwargs.get("num_return_sequences") not in (None, 1):
            raise NotImplementedError("num_return_sequences > 1 is not supported")
        gen: GenerationConstants = copy.deepcopy(generation_config or self.generation_config)
        if isinstance(gen, dict):
            gen = GenerationConstants(**gen)
        num_beams = kwargs.get("num_beams", gen.num_beams or 1)
        repeat = _repeat_arguments(kwargs, gen)
        seq_tables = _sequence_arguments(kwargs, gen, self.engine.shape.vocab_size)
        # decoding fallback: the thresholds from the call or the generation config (_set_thresholds_and_condition,
        # generation_whisper.py:1703-1729) and the temperature schedule (:735); `do_sample` itself is overridden by
        # the schedule (:1002-1010)
        thr = {k: kwargs.get(k) if kwargs.get(k) is not None else getattr(gen, k, None)
               for k in ("compression_ratio_threshold", "logprob_threshold", "no_speech_threshold")}
        cond_prev = kwargs.get("condition_on_prev_tokens")
        if cond_prev is None:
            cond_prev = getattr(gen, "condition_on_prev_tokens", None)
        gen.condition_on_prev_tokens = cond_prev
        # _set_prompt_condition_type (generation_whisper.py:1732-1748)
        prompt_condition_type = kwargs.get("prompt_condition_type") or "first-segment"
        if prompt_condition_type not in ("first-segment", "all-segments"):
            raise ValueError(
                f"`prompt_condition_type={prompt_condition_type} does not exist. Make sure to set "
                "`prompt_condition_type` to one of first-segment, all-segments")
        if cond_prev is not True and prompt_condition_type == "all-segments":
            raise ValueError(
                "Make sure to set `condition_on_prev_tokens=True` when setting `prompt_condition_type='all-segments'`.")
        cond_prev = bool(cond_prev)
        prompt_ids = kwargs.get("prompt_ids")
        if prompt_ids is not None:
            prompt_ids = (prompt_ids.detach().cpu().numpy() if isinstance(prompt_ids, torch.Tensor)
                          else np.asarray(prompt_ids)).astype(np.int64)
            if prompt_ids.ndim != 1 or prompt_ids.size == 0:
                raise ValueError("`prompt_ids` must be a non-empty rank-1 tensor of token ids")
        prompted = prompt_ids is not None or cond_prev
        temperature = kwargs.get("temperature")
        temperatures = list(temperature) if isinstance(temperature, (list, tuple)) else [temperature]
        has_thr = any(v is not None for v in thr.values())
        fallback = has_thr or any(t is not None and t > 0.0 for t in temperatures)
        if fallback:
            if thr["no_speech_threshold"] is not None and thr["logprob_threshold"] is None:
                raise ValueError("`no_speech_threshold` needs `logprob_threshold`: a window is skipped only when its "
                                 "average log-probability is below `logprob_threshold` as well")
            temperatures = [0.0 if t is None else float(t) for t in temperatures]
            if not temperatures:
                raise ValueError("`temperature` must be a number or a non-empty sequence of numbers")
            if num_beams > 1:
                raise NotImplementedError("the decoding fallback (thresholds or a temperature above 0) with `num_beams` "
                                          "> 1 is not supported by the MI355X engine yet; use num_beams=1")
            if kwargs.get("return_token_timestamps"):
                raise NotImplementedError("the decoding fallback (thresholds or a temperature above 0) with "
                                          "`return_token_timestamps` is not supported by the MI355X engine yet")
        if prompted:
            if num_beams > 1:
                raise NotImplementedError("`prompt_ids` / `condition_on_prev_tokens` with `num_beams` > 1 is not "
                                          "supported by the MI355X engine yet; use num_beams=1")
            if kwargs.get("return_token_timestamps"):
                raise NotImplementedError("`prompt_ids` / `condition_on_prev_tokens` with `return_token_timestamps` is "
                                          "not supported by the MI355X engine yet (the alignment log is not extended to "
                                          "padded prompts)")
        if num_beams > 8:
            raise NotImplementedError("num_beams > 8 is not supported by the device beam search")
        if getattr(self.engine, "cross_kv_fp8", False):
            if num_beams > 1:
                raise NotImplementedError("`num_beams` > 1 is not supported with cross_kv_dtype='fp8_e4m3' (the fp8 "
                                          "cross-attention has no beam kernel); use num_beams=1 or the bf16 cache")
            if kwargs.get("return_token_timestamps"):
                raise NotImplementedError("`return_token_timestamps` is not supported with cross_kv_dtype='fp8_e4m3' "
                                          "(the alignment weights read the bf16 K cache); use the bf16 cache")
        # assisted (speculative) generate: the assistant drafts, this model verifies -- its own greedy tokens
        assistant = kwargs.get("assistant_model")
        num_assist = 0
        if assistant is not None:
            num_assist = _assistant_arguments(self, assistant, kwargs, num_beams=num_beams, fallback=fallback,
                                              prompted=prompted, repeat=repeat, seq_tables=seq_tables)
            gen.begin_suppress_tokens = None  # dropped with an assistant (generation_whisper.py:718-720)
        length_penalty = kwargs.get("length_penalty", getattr(gen, "length_penalty", 1.0))
        early_stopping = kwargs.get("early_stopping", getattr(gen, "early_stopping", False))
        max_new_tokens = kwargs.get("max_new_tokens")
        max_length = kwargs.get("max_length", gen.max_length)
        s = self.engine.shape
        eng = self.engine
        # token timestamps (_set_num_frames, generation_whisper.py:1685-1700)
        token_ts = bool(kwargs.get("return_token_timestamps"))
        align = ts_frames = None
        if token_ts:
            if getattr(gen, "alignment_heads", None) is None:
                raise ValueError(
                    "Model generation config has no `alignment_heads`, token-level timestamps not available. "
                    "See https://gist.github.com/hollance/42e32852f24243b748ae6bc1f985b13a on how to add this property "
                    "to the generation config.")
            if num_beams > 1 and not getattr(self.engine, "beam_token_ts", False):
                # (asked of the engine before anything touches the device, like the fp8 checks above: beam sessions
                # that log every running row's queries and record the beam parents are WhisperEngine.beam_token_ts)
                raise NotImplementedError(
                    "`return_token_timestamps` with `num_beams` > 1 needs an engine whose beam sessions keep the "
                    "alignment log and the beam parents (`beam_token_ts`), which this engine does not declare; use "
                    "greedy decoding")
            align = [tuple(p) for p in gen.alignment_heads]
            if attention_mask is not None:
                ts_frames = torch.as_tensor(attention_mask).sum(-1).cpu().long().numpy()

        enc_given = kwargs.get("encoder_outputs")
        if input_features is None and enc_given is None:
            raise ValueError("Make sure to provide either `input_features` or `encoder_outputs` to `generate`.")
        if input_features is not None:
            feats = input_features.to(device=eng.device, dtype=torch.float32)
            B, total = feats.shape[0], feats.shape[-1]
        else:
            eh = enc_given.last_hidden_state if hasattr(enc_given, "last_hidden_state") else enc_given[0] \
                if isinstance(enc_given, (tuple, list)) else enc_given
            B, total = eh.shape[0], eh.shape[1] * 2
            feats = None
        if assistant is not None:
            if B > 1:
                raise ValueError("assisted generate is only supported for batch_size = 1")
            if feats is None:
                raise NotImplementedError("`assistant_model` with `encoder_outputs` is not supported by the MI355X "
                                          "engine yet (the assistant encodes the features with its own encoder)")
        assisted = {"rounds": 0, "drafted": 0, "accepted": 0}
        nseg = s.n_frames
        shortform = total <= nseg
        if prompted and fallback and shortform:
            raise NotImplementedError("`prompt_ids` / `condition_on_prev_tokens` together with the decoding fallback "
                                      "(thresholds or a temperature above 0) is supported for long-form input (more than "
                                      "one 30 s window) only; it is not supported for short-form input by the MI355X "
                                      "engine yet")
        if return_timestamps is None:
            return_timestamps = bool(getattr(gen, "return_timestamps", False))
        if not shortform:
            if return_timestamps is False:
                raise ValueError(
                    "You have passed more than 3000 mel input features (> 30 seconds) which automatically enables "
                    "long-form generation which requires the model to predict timestamp tokens. Please either pass "
                    "`return_timestamps=True` or make sure to pass no more than 3000 mel input features.")
            return_timestamps = True
        if return_dict_in_generate is None:
            return_dict_in_generate = False
        if is_multilingual is not None:
            gen.is_multilingual = is_multilingual
        if not gen.is_multilingual and (task is not None or language is not None):
            raise ValueError("Cannot specify `task` or `language` for an English-only model.")

        # prompt (init tokens)
        self._sot_logits = None
        prompt_all = self._init_tokens(gen, B, language, task, return_timestamps, feats, enc_given)
        P = prompt_all.shape[1]

        if not prompted and max_new_tokens is not None and max_new_tokens + P > s.max_target_positions:
            raise ValueError(
                f"The length of `decoder_input_ids`, including special start tokens, prompt tokens, and previous "
                f"tokens, is {P},  and `max_new_tokens` is {max_new_tokens}. Thus, the combined length of "
                f"`decoder_input_ids` and `max_new_tokens` is: {max_new_tokens + P}. This exceeds the "
                f"`max_target_positions` of the Whisper model: {s.max_target_positions}. You should either reduce "
                "the length of your prompt, or reduce the value of `max_new_tokens`, so that their combined length "
                f"is less than {s.max_target_positions}.")
        if not shortform and B > 1:
            if attention_mask is None:
                raise ValueError(
                    "When doing batched long-form audio transcription, make sure to pass an `attention_mask`. You "
                    "can retrieve the `attention_mask` by doing `processor(audio, ..., return_attention_mask=True)` ")
            max_frames = attention_mask.sum(-1).cpu().long().numpy()
        else:
            max_frames = np.full(B, total, dtype=np.int64)
        seek = np.zeros(B, dtype=np.int64)
        ts_begin = gen.timestamp_begin
        # _prepare_segments (:1119-1126): "first-segment" seeds every row's segments with the prompt's text
        first_seg = prompt_ids is not None and prompt_condition_type == "first-segment"
        if first_seg:
            seed = prompt_ids[1:] if prompt_ids[0] == gen.prev_sot_token_id else prompt_ids
            segments = [[{"tokens": seed}] for _ in range(B)]
        else:
            segments = [[] for _ in range(B)]
        do_condition = [cond_prev] * B  # per audio, for its next pass (_expand_variables_for_generation :1304)
        pass_P, pass_key_start, pass_prompt = [], [], []
        batch_map = list(range(B))
        last_ids = None
        passes = 0
        row_passes = np.zeros(B, dtype=np.int64)
        pass_log, pass_ids = [], []  # per pass: (rows, their seek, their frame count); the decoded ids
        align_log, last_ts = [], None
        fallback_log = []
        while (seek < max_frames).any():
            batch_map = [p for p in batch_map if seek[p] < max_frames[p]]
            cur = len(batch_map)
            row_passes[batch_map] += 1
            time_offset = seek.astype(np.float64) * 0.02 / 2
            seek_num = np.minimum(max_frames - seek, nseg)
            if feats is not None:
                whole = shortform and total == nseg and all(seek[p] == 0 for p in batch_map) and cur == B
                if whole:
                    seg_in = feats
                else:
                    seg_in = torch.zeros((cur, feats.shape[1], nseg), device=eng.device, dtype=torch.float32)
                    for i, p in enumerate(batch_map):
                        n = int(seek_num[p])
                        seg_in[i, :, :n] = feats[p, :, int(seek[p]): int(seek[p]) + n]
                enc_key = None
                memo = self._memo
                if memo is not None and whole and passes == 0:
                    # multi-task reuse: the first pass of every prompt sees the same mel, so the encoder and
                    # the cross-K/V projection run once per batch (clone: later passes reuse the buffer)
                    if "enc" not in memo:
                        memo["enc"] = eng.encode(seg_in).clone()
                    enc, enc_key = memo["enc"], ("memo", memo["id"])
                else:
                    enc = eng.encode(seg_in)
            else:
                if passes > 0:
                    raise NotImplementedError("encoder_outputs with a multi-pass seek loop")
                enc = eh.to(eng.device, eng.dtype).reshape(B * s.max_source_positions, s.d_model).contiguous()
                enc_key = None
            prompt = prompt_all[batch_map]
            key_start = None
            if prompted:
                # this pass's decoder input and per-row first key; the same for every attempt of the fallback
                prompt, key_start = build_pass_input(prompt_all, segments, batch_map, do_condition, prompt_ids, gen,
                                                     s.max_target_positions, prompt_condition_type)
                P = prompt.shape[1]
                # _set_max_new_tokens_and_length (:1920-1945), with this pass's length
                if (max_new_tokens or 0) + P > s.max_target_positions:
                    raise ValueError(
                        f"The length of `decoder_input_ids`, including special start tokens, prompt tokens, and previous "
                        f"tokens, is {P},  and `max_new_tokens` is {max_new_tokens or 0}. Thus, the combined length of "
                        f"`decoder_input_ids` and `max_new_tokens` is: {(max_new_tokens or 0) + P}. This exceeds the "
                        f"`max_target_positions` of the Whisper model: {s.max_target_positions}. You should either reduce "
                        "the length of your prompt, or reduce the value of `max_new_tokens`, so that their combined length "
                        f"is less than {s.max_target_positions}.")
            pass_P.append(int(P))
            pass_key_start.append(None if key_start is None else [int(k) for k in key_start])
            if self.record_pass_ids:
                pass_prompt.append((np.asarray(prompt).copy(), list(do_condition)))
            if max_new_tokens is None:
                max_length = min(max_length + min(s.max_target_positions // 2 - 1, P), s.max_target_positions)
                eff_max = max_length
            else:
                eff_max = P + max_new_tokens
            if assistant is not None:
                # the assistant encodes the pass's features with its own encoder; the paired session decodes the row
                sess = self._spec_session(assistant)
                sess.set_encoder_output(enc, assistant.engine.encode(seg_in))
            else:
                sess = self._session(cur, num_beams)
                sess.set_encoder_output(enc, key=enc_key)
            skip = [False] * cur
            rep_kw = {} if repeat is None else {"repeat": repeat}  # (None: the session calls as they ever were)
            if seq_tables is not None:
                rep_kw["seq_tables"] = seq_tables
            if assistant is not None:
                ids = sess.generate(torch.from_numpy(prompt), gen, K=num_assist, max_length=eff_max,
                                    return_timestamps=return_timestamps)
                for k in assisted:
                    assisted[k] += int(sess.last_stats[k])
            elif fallback:
                sot = None
                if passes == 0 and feats is not None and whole and self._sot_logits is not None \
                        and self._sot_logits.shape[0] == cur:
                    sot = self._sot_logits  # language detection ran this very position on these features
                ids, skip, attempts = self._generate_with_fallback(sess, prompt, gen, eff_max, return_timestamps,
                                                                   temperatures, thr, batch_map, sot, key_start, repeat,
                                                                   seq_tables)
                fallback_log.append(attempts)
                for rec in attempts:  # (:1088-1093): a row accepted at a temperature of 0.5 or more loses its conditioning
                    for p in rec["rows"]:
                        do_condition[p] = cond_prev and rec["temperature"] < 0.5
            elif num_beams > 1 and not token_ts:
                ids = sess.generate_beam(torch.from_numpy(prompt), gen, num_beams=num_beams, max_length=eff_max,
                                         return_timestamps=return_timestamps, length_penalty=length_penalty,
                                         early_stopping=early_stopping, **rep_kw)
            elif token_ts:
                # per pass: num_frames - seek of the rows still running (generation_whisper.py:1146-1150)
                nf = None if ts_frames is None else [int(ts_frames[p] - seek[p]) for p in batch_map]
                sess.keep_alignment = self.record_alignment
                ts_kw = dict(rep_kw, max_length=eff_max, return_timestamps=return_timestamps, align=align, num_frames=nf,
                             median_filter_width=s.median_filter_width)
                if num_beams > 1:
                    # the returned hypotheses' steps are gathered from the running rows that produced them
                    # (beam_indices, generation_whisper.py:265-301); every row gets P + longest hypothesis times
                    ids = sess.generate_beam(torch.from_numpy(prompt), gen, num_beams=num_beams,
                                             length_penalty=length_penalty, early_stopping=early_stopping, **ts_kw)
                else:
                    ids = sess.generate(torch.from_numpy(prompt), gen, **ts_kw)
                pass_ts = _pass_token_timestamps(sess.align_out["frames"], P, ids.shape[1])
                if self.record_alignment:
                    align_log.append(dict(sess.align_out, rows=[int(p) for p in batch_map], num_input_ids=P))
            else:
                ids = sess.generate(torch.from_numpy(prompt), gen, max_length=eff_max,
                                    return_timestamps=return_timestamps, key_start=key_start, **rep_kw)
            passes += 1
            last_ids = ids
            pass_log.append(([int(p) for p in batch_map], [int(seek[p]) for p in batch_map],
                             [int(seek_num[p]) for p in batch_map]))
            if self.record_pass_ids:
                pass_ids.append(np.asarray(ids).copy())
            pad, eos = gen.pad_token_id, gen.eos_token_id
            for i, p in enumerate(batch_map):
                if skip[i]:  # a no-speech window: no segment, the seek moves on (generation_whisper.py:876-881)
                    seek[p] += seek_num[p]
                    continue
                seq = _strip_pass_row(ids[i, P:], pad, eos)
                segs, off = _retrieve_segment(seq, ts_begin, int(seek_num[p]), float(time_offset[p]),
                                              token_ts=(pass_ts[i], ids[i], P) if token_ts else None)
                seek[p] += off
                segments[p] += segs
            if token_ts:
                last_ts = pass_ts
        if first_seg:  # the seeded prompt is no part of the result (:905-915)
            segments = [x[1:] for x in segments]
        self.stats = {"passes": passes, "row_passes": row_passes, "pass_log": pass_log, "pass_P": pass_P,
                      "pass_key_start": pass_key_start}
        if self.record_pass_ids:
            self.stats["pass_ids"] = pass_ids
            self.stats["pass_prompt"] = pass_prompt
        if token_ts and self.record_alignment:
            self.stats["alignment"] = align_log
        if fallback:
            self.stats["fallback"] = fallback_log
        if assistant is not None:
            self.stats["assisted"] = assisted
        if return_dict_in_generate and not return_timestamps:
            res = {"sequences": torch.from_numpy(last_ids).to(eng.device)}
            if token_ts:  # _stack_split_outputs: the single pass's timestamps, prompt positions included
                res["token_timestamps"] = torch.from_numpy(last_ts).to(eng.device)
            return res
        seqs = [np.concatenate([x["tokens"] for x in segs]) if segs else np.zeros(0, np.int64) for segs in segments]
        longest = max(len(x) for x in seqs) if seqs else 0
        out = np.full((B, longest), gen.pad_token_id, dtype=np.int64)
        for i, x in enumerate(seqs):
            out[i, : len(x)] = x
        res = torch.from_numpy(out).to(eng.device)
        if token_ts:
            # _pad_to_max_length (:188-229): each segment's slice of its pass's timestamps (no time offset), padded
            # with the row's last value
            tts = _pad_token_timestamps(segments, longest)
            ret = {"sequences": res, "token_timestamps": torch.from_numpy(tts).to(eng.device)}
            if return_segments or (return_dict_in_generate and return_timestamps):
                ret["segments"] = segments
            return ret
        if return_segments or (return_dict_in_generate and return_timestamps):
            return {"sequences": res, "segments": segments}
        return res

    def _generate_with_fallback(self, sess, prompt, gen, max_length, return_timestamps, temperatures, thr, batch_map,
                                sot_logits=None, key_start=None, repeat=None, seq_tables=None):
        """One seek pass's attempt loop (``generate_with_fallback``, generation_whisper.py:1001-1116): decode at each
        temperature of the schedule in turn -- 0 greedy, above 0 sampled -- re-decoding only the rows whose
        ``_need_fallback`` decision asks for it, in the same session (its cross K/V stays; no re-encode); the last
        temperature's result is accepted.  Returns the pass's ids (cur, L) with every row from the attempt that was
        accepted for it (right-padded), the rows to skip, and the per-attempt record kept in ``stats["fallback"]``.
        ``repeat`` and ``seq_tables`` go to every attempt (the reference copies the generation config per attempt)."""
        cur, P = prompt.shape
        pad, eos, V = gen.pad_token_id, gen.eos_token_id, self.engine.shape.vocab_size
        nsp = None
        if thr["no_speech_threshold"] is not None:
            nsp = sess.no_speech_prob(gen.decoder_start_token_id, gen.no_timestamps_token_id - 1, sot_logits)
        rows = list(range(cur))
        final = [None] * cur
        skip = [False] * cur
        attempts = []
        for ai, t in enumerate(temperatures):
            if t > 0.0:
                self._attempts += 1
            active = np.zeros(cur, bool)
            active[rows] = True
            ids = sess.generate(torch.from_numpy(prompt), gen, max_length=max_length, return_timestamps=return_timestamps,
                                **({} if key_start is None else {"key_start": key_start}),
                                **({} if repeat is None else {"repeat": repeat}),
                                **({} if seq_tables is None else {"seq_tables": seq_tables}),
                                sample=dict(temperature=t, seed=self._seed, active=active,
                                            attempt=(self._lane << 24) | (self._attempts & 0xFFFFFF)))
            rec = dict(rows=[int(batch_map[i]) for i in rows], temperature=float(t), avg_logprob=[], compression_ratio=[],
                       no_speech_prob=[], needs_fallback=[], should_skip=[])
            again = []
            for i in rows:
                # the row's tokens without the padding but with its EOS (:1063-1071)
                seq = _strip_pass_row(ids[i, P:], pad, eos, keep_eos=True)
                cr = _compression_ratio(seq, V) if thr["compression_ratio_threshold"] is not None else None
                lp = float(sess.avg_logprob[i])
                p_ns = float(nsp[i]) if nsp is not None else None
                needs, skips = _need_fallback(cr, lp, p_ns, thr)
                for k, v in (("avg_logprob", lp), ("compression_ratio", cr), ("no_speech_prob", p_ns),
                             ("needs_fallback", needs), ("should_skip", skips)):
                    rec[k].append(v)
                final[i], skip[i] = ids[i], skips
                if needs:
                    again.append(i)
            attempts.append(rec)
            rows = again
            if not rows:
                break
        longest = max(len(r) for r in final)
        out = np.full((cur, longest), pad, dtype=np.int64)
        for i, r in enumerate(final):
            out[i, : len(r)] = r
        return out, skip, attempts

    def generate_multitask(self, input_features, tasks, **kwargs):
        """``generate`` once per (language, task) of ``tasks`` on the same features -- the inner loop of
        run_pseudo_labelling_v3.py:309-318 -- with ONE encoder pass and ONE cross-K/V projection shared by
        every prompt.  Each result is exactly what ``generate(input_features,
        language=..., task=..., **kwargs)`` returns on its own; only passes after the first (the
        timestamp seek loop's re-encodes of shifted mel) run the encoder again."""
        if not tasks:
            return []
        for k in ("language", "task", "encoder_outputs"):
            if k in kwargs:
                raise ValueError(f"generate_multitask takes `{k}` from `tasks`, not as a keyword")
        self._memo_count += 1
        self._memo = {"id": self._memo_count}
        try:
            return [self.generate(input_features, language=lang, task=task, **kwargs) for lang, task in tasks]
        finally:
            self._memo = None

    # ---- helpers ------------------------------------------------------------------------------------
    def detect_language(self, input_features=None, encoder_outputs=None, generation_config=None):
        """``detect_language`` (generation_whisper.py:1620-1674)."""
        gen = generation_config or self.generation_config
        eng = self.engine
        if input_features is not None:
            B = input_features.shape[0]
            enc = eng.encode(input_features[:, :, : eng.shape.n_frames].to(eng.device, torch.float32))
        else:
            eh = encoder_outputs.last_hidden_state if hasattr(encoder_outputs, "last_hidden_state") else encoder_outputs
            B = eh.shape[0]
            enc = eh.to(eng.device, eng.dtype).reshape(B * eng.shape.max_source_positions, eng.shape.d_model)
        sess = self._session(B)
        sess.set_encoder_output(enc)
        prompt = torch.full((B, 1), gen.decoder_start_token_id, dtype=torch.int64, device=eng.device)
        logits = sess.forward_logits(prompt).clone()
        self._sot_logits = logits.clone()
        mask = torch.ones(logits.shape[-1], dtype=torch.bool, device=logits.device)
        mask[list(gen.lang_to_id.values())] = False
        logits[:, mask] = -float("inf")
        return logits.argmax(-1)

    def _init_tokens(self, gen, B, language, task, return_timestamps, feats, enc_given):
        """``_retrieve_init_tokens`` (generation_whisper.py:1455-1608) for the task/language API."""
        if language is None and getattr(gen, "language", None) is not None:
            language = gen.language
        if task is None and getattr(gen, "task", None) is not None:
            task = gen.task
        if isinstance(language, (list, tuple)):
            if any(x is None for x in language):
                raise TypeError("Expected `language` to be `None`, a single string (e.g. `'en'`), or a list of "
                                "strings with length equal to the batch size (e.g. `('en', 'fr')` for a batch size "
                                "of 2). Got a list containing `None`.")
            if len(language) != B:
                raise ValueError("When passing a list of languages, the length of the list must match the batch "
                                 f"size. Expected length of {B}, but got {len(language)} languages.")
            langs = list(language)
        elif language is None:
            langs = [None] * B
        else:
            langs = [language]
        rows = [[gen.decoder_start_token_id] for _ in langs]
        lang_ids = None
        if language is not None:
            lang_ids = [language_to_id(x, gen) for x in langs]
        elif gen.lang_to_id:
            lang_ids = self.detect_language(feats, enc_given if feats is None else None, gen).tolist()
        if lang_ids is not None:
            for i in range(len(rows)):
                rows[i].append(int(lang_ids[i]))
        if task is not None and task not in ("translate", "transcribe"):
            raise ValueError(f"The `{task}` task is not supported. The task should be one of `['translate', 'transcribe']`")
        for r in rows:
            if task is not None:
                r.append(gen.task_to_id[task])
            elif language is not None and gen.task_to_id:
                if not any(t in r for t in gen.task_to_id.values()):
                    r.append(gen.task_to_id["transcribe"])
            if not return_timestamps and r[-1] != gen.no_timestamps_token_id:
                r.append(gen.no_timestamps_token_id)
            elif return_timestamps and r[-1] == gen.no_timestamps_token_id:
                r.pop()
        arr = np.asarray(rows, dtype=np.int64)
        return np.broadcast_to(arr, (B, arr.shape[1])).copy()


def _assistant_arguments(model, assistant, kwargs, *, num_beams, fallback, prompted, repeat, seq_tables=None) -> int:
    """Check an ``assistant_model`` call and return K, the constant number of tokens drafted per round: from the call
    (``num_assistant_tokens``), else the assistant's generation config, else 5."""
    if not isinstance(assistant, KWhisperForConditionalGeneration):
        raise NotImplementedError("`assistant_model` must be a KWhisperForConditionalGeneration (both decoders run on "
                                  "the MI355X engine); other assistants are not supported")
    for on, what in ((num_beams > 1, "`num_beams` > 1"),
                     (fallback, "the decoding fallback (thresholds or a temperature above 0)"),
                     (bool(kwargs.get("return_token_timestamps")), "`return_token_timestamps`"),
                     (prompted, "`prompt_ids` / `condition_on_prev_tokens`"),
                     (repeat is not None, "`repetition_penalty` / `no_repeat_ngram_size`"),
                     (seq_tables is not None, "`sequence_bias` / `bad_words_ids`"),
                     (getattr(model.engine, "cross_kv_fp8", False) or getattr(assistant.engine, "cross_kv_fp8", False),
                      "cross_kv_dtype='fp8_e4m3'")):
        if on:
            raise NotImplementedError(f"`assistant_model` together with {what} is not supported by the MI355X engine "
                                      "yet")
    if assistant.engine.shape.vocab_size != model.engine.shape.vocab_size:
        raise ValueError("Make sure the main and assistant model use the same tokenizer: their vocabularies differ "
                         f"({model.engine.shape.vocab_size} vs {assistant.engine.shape.vocab_size} tokens)")
    K = kwargs.get("num_assistant_tokens")
    if K is None:
        K = getattr(assistant.generation_config, "num_assistant_tokens", None)
    if K is None:
        K = 5
    if not isinstance(K, int) or isinstance(K, bool) or not 1 <= K <= 31:
        raise ValueError(f"`num_assistant_tokens` has to be an integer in [1, 31], but is {K}")
    return K


def _sequence_arguments(kwargs, gen, vocab_size):
    """``sequence_bias`` / ``bad_words_ids`` from the call, else the generation config, as the ``seq_tables`` pair of
    ``DecodeSession.generate`` -- None when neither processor would be built (TF generation/utils.py:1154-1155,
    1207-1213).  The values are checked as the processors check them (``ValueError``), token ids against the
    vocabulary as their first call does, the sizes against the engine's caps (``NotImplementedError``); bad words
    equal to ``[eos]`` are dropped, and a list that ends empty is no argument."""
    sb = kwargs.get("sequence_bias")
    if sb is None:
        sb = getattr(gen, "sequence_bias", None)
    bw = kwargs.get("bad_words_ids")
    if bw is None:
        bw = getattr(gen, "bad_words_ids", None)
    if sb is None and bw is None:
        return None
    sb, bw = seq_bias.build_tables(sb, bw, gen.eos_token_id, vocab_size)
    return None if sb is None and bw is None else (sb, bw)


def _repeat_arguments(kwargs, gen):
    """``repetition_penalty`` / ``no_repeat_ngram_size`` from the call, else the generation config, as the ``repeat``
    pair of ``DecodeSession.generate`` -- None when neither processor would be built (TF generation/utils.py:1174-1183:
    a penalty of None or 1.0, an n-gram size of None or 0)."""
    penalty = kwargs.get("repetition_penalty")
    if penalty is None:
        penalty = getattr(gen, "repetition_penalty", None)
    ngram = kwargs.get("no_repeat_ngram_size")
    if ngram is None:
        ngram = getattr(gen, "no_repeat_ngram_size", None)
    if penalty is not None and penalty != 1.0:
        # RepetitionPenaltyLogitsProcessor.__init__ (TF generation/logits_process.py:390-392)
        if not isinstance(penalty, float) or not (penalty > 0):
            raise ValueError(f"`penalty` has to be a strictly positive float, but is {penalty}")
    else:
        penalty = 1.0
    # (utils.py:1182: the processor is built for a size that is not None and > 0; its own check wants an int)
    if ngram is not None and ngram > 0:
        if not isinstance(ngram, int):
            raise ValueError(f"`ngram_size` has to be a strictly positive integer, but is {ngram}")
        ngram = int(ngram)
    else:
        ngram = 0
    return None if (penalty == 1.0 and ngram == 0) else (penalty, ngram)


def build_pass_input(init_tokens, segments, batch_map, do_condition, prompt_ids, gen, max_target_positions,
                     prompt_condition_type="first-segment"):
    """One seek pass's ``decoder_input_ids`` and per-row first key, in numpy: ``_prepare_decoder_input_ids``
    (generation_whisper.py:1853-1918) with the left-padding ``_pad_to_max_length`` (:126-235).

    ``init_tokens`` (B, n) int64; ``segments``: per audio, its segments so far (dicts with ``tokens``; with
    "first-segment" the first one is the prompt's text); ``batch_map``: the audios still running, in row order;
    ``do_condition``: per audio, whether its next pass sees its previous text; ``prompt_ids``: rank-1 or None.
    Returns (ids (rows, P) int64, key_start): key_start[r] is the number of leading positions of row r equal to
    ``pad_token_id`` -- the mask is ``ids != pad_token_id`` as at :1908 -- or None where the reference passes no mask.
    """
    ids = np.asarray(init_tokens, dtype=np.int64)[list(batch_map)]
    pad = gen.pad_token_id
    prev_sot = getattr(gen, "prev_sot_token_id", None)
    if prev_sot is None and gen.suppress_tokens is not None and len(gen.suppress_tokens) >= 2:
        prev_sot = gen.suppress_tokens[-2]
    if any(do_condition) and len(segments[0]) > 0:
        cut = max_target_positions // 2 - 1
        if prompt_ids is not None and prompt_condition_type == "all-segments":
            bos = np.asarray(prompt_ids, dtype=np.int64)
        else:
            bos = np.asarray([prev_sot], dtype=np.int64) if prev_sot is not None else None
        rows = []
        for p in batch_map:
            segs = segments[p] if do_condition[p] else None
            if segs is not None and len(segs) > 0:
                # a segment that ends with two timestamps gives only the first of them (skip_ending_double_timestamps)
                toks = [np.asarray(g["tokens"], dtype=np.int64) for g in segs]
                toks = [t[:-1] if len(t) > 2 and t[-2] >= gen.timestamp_begin else t for t in toks]
                row = np.concatenate(toks)[-cut:]
                if bos is not None:
                    row = np.concatenate([bos, row])
            else:
                row = bos if bos is not None else np.zeros(0, np.int64)
            rows.append(row)
        longest = max(len(r) for r in rows)
        prev = np.full((len(rows), longest), pad, dtype=np.int64)
        for r, row in enumerate(rows):
            prev[r, longest - len(row):] = row
        ids = np.concatenate([prev, ids], axis=1)
        keep = ids != pad
        key_start = np.where(keep.any(1), keep.argmax(1), ids.shape[1]).astype(np.int64)
        return ids, key_start
    if prompt_ids is not None:
        ids = np.concatenate([np.broadcast_to(np.asarray(prompt_ids, dtype=np.int64), (ids.shape[0], len(prompt_ids))),
                              ids], axis=1)
    return ids, None


def _strip_pass_row(seq, pad, eos, keep_eos=False):
    """A pass's generated tokens of one row without its padding and its EOS (generation_whisper.py:1063-1086);
    ``keep_eos``: with the EOS, as ``_need_fallback`` takes them."""
    if seq.size and seq[-1] == pad:
        n = int((seq == pad).sum())
        if pad == eos:
            n -= 1
        if n != 0:
            seq = seq[:-n]
    if not keep_eos and seq.size and seq[-1] == eos:
        seq = seq[:-1]
    return seq


def _compression_ratio(tokens, vocab_size):
    """``_retrieve_compression_ratio`` (generation_whisper.py:1949-1955): the tokens' bytes over their zlib size."""
    length = int(math.log2(vocab_size) / 8) + 1
    token_bytes = b"".join([int(t).to_bytes(length, "little") for t in tokens.tolist()])
    return len(token_bytes) / len(zlib.compress(token_bytes))


def _need_fallback(compression_ratio, avg_logprob, no_speech_prob, thr):
    """``_need_fallback`` (generation_whisper.py:1243-1287) on one row's numbers -> (needs_fallback, should_skip); a
    skip cancels a fallback."""
    needs_fallback = should_skip = False
    if thr["compression_ratio_threshold"] is not None and compression_ratio > thr["compression_ratio_threshold"]:
        needs_fallback = True
    if thr["logprob_threshold"] is not None and avg_logprob < thr["logprob_threshold"]:
        needs_fallback = True
    if thr["no_speech_threshold"] is not None:
        if avg_logprob < thr["logprob_threshold"] and no_speech_prob > thr["no_speech_threshold"]:
            needs_fallback = False
            should_skip = True
    return needs_fallback, should_skip


def _pad_token_timestamps(segments, longest):
    """The top-level ``token_timestamps`` (B, longest) float32 (_pad_to_max_length, :188-229): every segment's slice
    of its pass's timestamps (no time offset), right-padded with the row's last value."""
    tts = np.zeros((len(segments), longest), dtype=np.float32)
    for i, segs in enumerate(segments):
        x = np.concatenate([g["result"]["token_timestamps"][g["idxs"][0]: g["idxs"][1]] for g in segs]) \
            if segs else np.zeros(0, np.float32)
        tts[i, : len(x)] = x
        tts[i, len(x):] = x[-1] if len(x) else 0.0
    return tts


def _pass_token_timestamps(frames, num_input_ids, length):
    """One pass's ``_extract_token_timestamps`` result from the device's frame indices (B, T): float32 (B, length) =
    zeros for the prompt, frame * 0.02 per step, the last time once more (:306-308, :336-339, :368-379)."""
    B, T = frames.shape
    out = np.zeros((B, length), dtype=np.float32)
    if T > 0:
        jt = frames.astype(np.int64) * 0.02
        out[:, num_input_ids: num_input_ids + T] = jt
        out[:, num_input_ids + T] = jt[:, -1]
    return out


def _retrieve_segment(seq, ts_begin, seek_num_frames, time_offset, input_stride=2, time_precision=0.02,
                      time_precision_features=0.01, token_ts=None):
    """``_retrieve_segment`` (generation_whisper.py:1977-2074).  ``token_ts`` = (the row's per-pass token timestamps,
    its ids, the prompt length): segments then carry ``token_timestamps`` (their slice + time_offset), ``idxs`` and
    ``result`` as the reference's do."""
    segs, offset = _retrieve_segment_plain(seq, ts_begin, seek_num_frames, time_offset, input_stride, time_precision,
                                           time_precision_features)
    if token_ts is not None:
        row_ts, row_ids, P = token_ts
        result = {"sequences": row_ids, "token_timestamps": row_ts}
        last = 0
        for g in segs:
            n = len(g["tokens"])
            g["idxs"] = (P + last, P + last + n)
            g["result"] = result
            g["token_timestamps"] = row_ts[P + last: P + last + n] + np.float32(time_offset)
            last += n
    return segs, offset


def _retrieve_segment_plain(seq, ts_begin, seek_num_frames, time_offset, input_stride=2, time_precision=0.02,
                            time_precision_features=0.01):
    ts = seq >= ts_begin
    single_ending = ts[-2:].tolist() == [False, True]
    cons = np.where(ts[:-1] & ts[1:])[0] + 1
    if len(cons) > 0:
        slices = cons.tolist()
        if single_ending:
            slices.append(len(seq))
        else:
            slices[-1] += 1
        segs, last = [], 0
        for i, cur in enumerate(slices):
            is_last = i == len(slices) - 1
            st = seq[last:cur]
            start = int(st[0]) - ts_begin
            end = int(st[-1 if (not is_last or single_ending) else -2]) - ts_begin
            segs.append({"start": time_offset + start * time_precision, "end": time_offset + end * time_precision,
                         "tokens": st})
            last = cur
        offset = seek_num_frames if single_ending else (int(seq[last - 2]) - ts_begin) * input_stride
    else:
        stamps = seq[ts]
        last_pos = int(seek_num_frames * time_precision_features / time_precision)
        if stamps.size > 0 and stamps[-1] != ts_begin:
            last_pos = float(stamps[-1] - ts_begin)
        segs = [{"start": time_offset, "end": time_offset + last_pos * time_precision, "tokens": seq}]
        offset = seek_num_frames
    return segs, offset


# HF-style alias
WhisperForConditionalGeneration = KWhisperForConditionalGeneration
