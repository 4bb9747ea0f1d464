"""Host-side model handle over libsse.so: weights in, batched embeddings out.

``SSEModel`` is the perf surface of SURVEY.md §8(b):
``embed(wave[B, L]) -> [B, n_layers, H]`` (the fused mean-pooled output of
``extract_wavlm_embeddings`` / ``extract_whisper_embeddings_fixed`` for a whole batch),
plus ``hidden_states`` (the full HF-shaped tuple, materialised only on request).

Every tensor argument lives on the model's GPU; all compute runs in the HIP kernels of
``csrc/`` on the current torch stream.  There is no CPU path.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib
from .config import WavLMSpec, WhisperSpec, param_specs, resolve_frames

DTYPES = {"fp32": _lib.SSE_DTYPE_F32, "float32": _lib.SSE_DTYPE_F32, "f32": _lib.SSE_DTYPE_F32,
          "bf16": _lib.SSE_DTYPE_BF16, "bfloat16": _lib.SSE_DTYPE_BF16,
          "fp8": _lib.SSE_DTYPE_FP8, "mxfp8": _lib.SSE_DTYPE_FP8, "fp16x3": _lib.SSE_DTYPE_FP16X3,
          "fp16": _lib.SSE_DTYPE_FP16, "float16": _lib.SSE_DTYPE_FP16}
# fp8 / mxfp8: Whisper and stable-LN WavLM (WavLM-large); post-LN WavLM (WavLM-base) raises, see SSEModel
# dtypes whose activations live in the fp16 range: their calls are range-checked (sse_check_range)
FP16_RANGE = ("fp16", "float16", "fp16x3")


# statistics pooling: names of SSEModel.embed(pool=) -> sse_pool_desc.stats bits (output order mean, std, max)
POOL_STATS = {"mean": _lib.SSE_STAT_MEAN, "std": _lib.SSE_STAT_STD, "max": _lib.SSE_STAT_MAX}


def pool_mask(pool) -> int:
    """"mean" | "std" | "max" | "mean_std" | "mean_std_max" | a tuple of names -> the statistics bitmask."""
    names = pool.split("_") if isinstance(pool, str) else list(pool) if isinstance(pool, (tuple, list)) else None
    if not names or any(n not in POOL_STATS for n in names) or len(set(names)) != len(names):
        raise ValueError(f"pool must be one of mean, std, max, mean_std, mean_std_max or a tuple of those names, "
                         f"got {pool!r}")
    if isinstance(pool, str) and pool not in ("mean", "std", "max", "mean_std", "mean_std_max"):
        raise ValueError(f"unknown pool {pool!r} (pass a tuple of names for other combinations)")
    mask = 0
    for n in names:
        mask |= POOL_STATS[n]
    return mask


def pool_desc(pool="mean", window=None, hop=None, ddof=1, valid_only=False) -> _lib.sse_pool_desc:
    """Validate the pooling arguments (host only) and build the sse_pool_desc."""
    mask = pool_mask(pool)
    if ddof not in (0, 1):
        raise ValueError(f"ddof must be 0 or 1, got {ddof!r}")
    if (window is None) != (hop is None):
        raise ValueError("window and hop go together (both in frames)")
    win = 0
    if window is not None:
        win, hop = int(window), int(hop)
        if win <= 0 or hop <= 0 or win % hop:
            raise ValueError(f"window must be a positive multiple of hop, got window={window!r}, hop={hop!r}")
    return _lib.sse_pool_desc(mask, int(ddof), win, int(hop or 0), int(bool(valid_only)))


def _n_stats(desc) -> int:
    return bin(desc.stats).count("1")


def _as_numpy(v) -> np.ndarray:
    if isinstance(v, torch.Tensor):
        v = v.detach().to("cpu", torch.float32).numpy()
    return np.ascontiguousarray(np.asarray(v, dtype=np.float32))


def pack_weights(spec, state_dict: dict) -> np.ndarray:
    """Concatenate an HF state dict into the canonical fp32 blob (config.param_specs order).

    Accepts WavLMModel / WhisperModel state dicts (``encoder.``-prefixed keys for Whisper, as
    ``WhisperModel.state_dict()`` has them) with numpy arrays or torch tensors; the legacy
    ``weight_g`` / ``weight_v`` names of the WavLM pos-conv weight norm are mapped to the
    parametrization names.
    """
    sd = dict(state_dict)
    pre = "encoder.pos_conv_embed.conv."
    if pre + "weight_g" in sd and pre + "parametrizations.weight.original0" not in sd:
        sd[pre + "parametrizations.weight.original0"] = sd.pop(pre + "weight_g")
        sd[pre + "parametrizations.weight.original1"] = sd.pop(pre + "weight_v")
    parts = []
    for key, shape in param_specs(spec):
        if key.endswith("[0]") and key not in sd:        # row 0 of an embedding table
            base = key[:-3]
            if base not in sd:
                raise KeyError(f"state dict lacks {base}")
            v = sd[base]
            a = _as_numpy(v[0] if isinstance(v, torch.Tensor) else np.asarray(v)[0])
        elif key not in sd:
            raise KeyError(f"state dict lacks {key}")
        else:
            a = _as_numpy(sd[key])
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"{key}: shape {tuple(a.shape)} != expected {tuple(shape)}")
        parts.append(a.ravel())
    return np.concatenate(parts)


class SSEModel:
    """One model on one GPU.  ``dtype``: "bf16" (throughput path), "fp32" (parity path), "fp16x3"
    (WavLM-base: fp32 activations, split-fp16 GEMMs -- fp32-class parity at ~3x the fp32 path's
    throughput) or "fp8" (Whisper and stable-LN WavLM, i.e. WavLM-large: bf16 activations and residual
    stream, MX-fp8 QKV / fc1 / fc2 GEMMs, BASELINE configs[4]; post-LN WavLM (WavLM-base) is refused, it
    misses the fp8 bar on the format alone), "fp16" (WavLM-base: the bf16 path with fp16 activations and
    operands -- the same matrix-core rate, 8 more mantissa bits).

    A ``WavLMSpec`` with ``num_buckets=0`` (config.WAV2VEC2_* / HUBERT_*) is a wav2vec 2.0 / HuBERT encoder: the
    same network without the gated relative-position bias (no gate columns in the QKV GEMM, the bias-free
    attention kernels); every dtype rule above holds for it by shape (fp8: the stable-LN large shapes only).

    fp16 / fp16x3 keep activations in the fp16 range: with ``check_range`` (default) every embed /
    hidden_states call synchronises and raises ``SSERangeError`` if it produced a non-finite value
    (an overflow); throughput loops pass ``check_range=False`` and call ``check_range_now()`` once."""

    def __init__(self, spec, state_dict: dict, device="cuda:0", dtype: str = "bf16", do_normalize: bool = False,
                 check_range: bool = True):
        if not isinstance(spec, (WavLMSpec, WhisperSpec)):
            raise TypeError(spec)
        self.spec = spec
        if spec.hidden % spec.heads or spec.head_dim != 64:
            raise ValueError(f"{spec.name}: hidden / heads = {spec.hidden} / {spec.heads}: the attention kernels are "
                             f"built for a head width of 64 (hubert-xlarge and XLS-R-1B / 2B, head width 80 / 120, "
                             f"are out of scope)")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("SSEModel runs on a GPU device (no CPU fallback)")
        self.dtype = dtype
        self.do_normalize = bool(do_normalize)
        L = _lib.lib()
        self._cfg = _lib.make_cfg(spec, do_normalize)
        blob = pack_weights(spec, state_dict)
        need = L.sse_weight_floats(ctypes.byref(self._cfg))
        if need != blob.size:
            raise ValueError(f"weight blob has {blob.size} floats, library expects {need}")
        h = ctypes.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        torch.cuda.set_device(self.device)   # make sure the HIP context exists on this device
        rc = L.sse_model_create(ctypes.byref(self._cfg), blob.ctypes.data, blob.nbytes, idx, DTYPES[dtype],
                                ctypes.byref(h))
        if (rc == _lib.SSE_ERR_UNSUPPORTED and DTYPES[dtype] == _lib.SSE_DTYPE_FP8 and isinstance(spec, WavLMSpec)
                and not spec.stable_layer_norm):
            raise _lib.SSEError(rc, f"sse_model_create({spec.name}, dtype={dtype!r}): post-LN WavLM is not supported "
                                    f"in fp8 (its LayerNorms re-normalise the quantisation error into the stream at "
                                    f"every sub-layer: emulated 0.093 rel-L2 against the fp8 bar of 0.08, DESIGN.md §3); "
                                    f"use dtype='bf16' or 'fp16'")
        _lib.check(rc, "sse_model_create")
        self._h = h
        self._ws = None
        self.check_range = bool(check_range) and dtype in FP16_RANGE

    # -- plumbing -------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().sse_model_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def hidden_size(self) -> int:
        return self.spec.hidden

    def output_frames(self, n_samples: int, *, frames=None) -> int:
        F = resolve_frames(self.spec, frames, n_samples)
        return F if F is not None else _lib.lib().sse_output_frames(self._h, int(n_samples))

    def workspace_bytes(self, B: int, L: int, *, frames=None) -> int:
        """Device workspace a call on B clips of L samples needs; ``frames`` (Whisper audio context): every
        B * T term scales with it."""
        F = resolve_frames(self.spec, frames, L)
        if F is None:
            return int(_lib.lib().sse_workspace_bytes(self._h, int(B), int(L)))
        return int(_lib.lib().sse_workspace_bytes_ctx(self._h, int(B), int(L), F))

    def workspace(self, B: int, L: int, *, frames=None) -> torch.Tensor:
        n = self.workspace_bytes(B, L, frames=frames)
        if n == 0:
            raise _lib.SSEError(-1, f"sse_workspace_bytes(B={B}, L={L}, frames={frames})")
        if self._ws is None or self._ws.numel() < n:
            self._ws = None
            self._ws = torch.empty(n, dtype=torch.uint8, device=self.device)
        return self._ws

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def check_range_now(self) -> None:
        """Synchronise the current stream; raise SSERangeError if a call since the last check wrote a
        non-finite value (fp16 / fp16x3 models; a no-op for the others)."""
        _lib.check(_lib.lib().sse_check_range(self._h, self._stream()), "sse_check_range")

    def _after(self, check_range: bool | None = None):
        if self.check_range if check_range is None else (check_range and self.dtype in FP16_RANGE):
            self.check_range_now()

    def _check_wave(self, wave: torch.Tensor) -> torch.Tensor:
        if not isinstance(wave, torch.Tensor) or wave.device != self.device:
            raise ValueError(f"expected a tensor on {self.device}")
        if wave.dim() == 1:
            wave = wave[None]
        if wave.dim() != 2:
            raise ValueError("expected [B, L] waves")
        return wave.to(torch.float32).contiguous()

    # -- live launch timing (bench.py) ------------------------------------------------------
    def profile_start(self, max_launches: int = 8192) -> None:
        _lib.check(_lib.lib().sse_profile_start(self._h, int(max_launches)), "sse_profile_start")
        self._prof_cap = int(max_launches)

    def profile_read(self) -> list:
        """[(tag, ms, flops, bytes)] for every launch since profile_start / the last read."""
        cap = self._prof_cap
        tags = ctypes.create_string_buffer(32 * cap)
        ms = np.zeros(cap, np.float32)
        fl = np.zeros(cap, np.float64)
        by = np.zeros(cap, np.float64)
        n = _lib.lib().sse_profile_read(self._h, cap, tags, ms.ctypes.data, fl.ctypes.data, by.ctypes.data)
        if n < 0:
            _lib.check(n, "sse_profile_read")
        raw = tags.raw
        return [(raw[32 * i:32 * i + 32].split(b"\0", 1)[0].decode(), float(ms[i]), float(fl[i]), float(by[i]))
                for i in range(min(n, cap))]

    def profile_stop(self) -> None:
        _lib.check(_lib.lib().sse_profile_stop(self._h), "sse_profile_stop")

    # -- compute --------------------------------------------------------------------------
    def pool_segments(self, n_samples: int, window=None, hop=None, valid_only: bool = False, *, frames=None) -> int:
        """Segments embed(window=, hop=) fills for a clip of n_samples (the rest of its slots are zeros);
        ``frames``: the Whisper audio context of that embed call."""
        d = pool_desc("mean", window, hop, 1, valid_only)
        T = self.output_frames(n_samples, frames=frames)
        if d.valid_only and isinstance(self.spec, WhisperSpec):
            T = min(T, -(-int(n_samples) // 320))
        if T <= 0:
            return 0
        return int(_lib.lib().sse_pool_segments(int(T), d.win, d.hop))

    def embed(self, wave: torch.Tensor, layer_indices, out: torch.Tensor | None = None,
              lengths=None, workspace: torch.Tensor | None = None, check_range: bool | None = None, *,
              pool="mean", window=None, hop=None, ddof: int = 1, valid_only: bool = False,
              frames=None) -> torch.Tensor:
        """[B, L] fp32 16 kHz waves -> [B, len(layer_indices), H] fp32 time-means of hidden states.
        ``lengths`` (ragged batch): samples of each clip, its first lengths[b] samples of row b; each
        clip is embedded at its own length (sse_embed_ragged).  ``check_range`` overrides the model's
        per-call fp16-range check (False in throughput loops, which call check_range_now() once).

        Statistics pooling (sse_embed_pooled): ``pool`` = "mean" | "std" | "max" | "mean_std" |
        "mean_std_max" | a tuple of names selects the statistics, concatenated in the order mean, std, max
        -> [B, n_layers, n_stats*H]; std is ``torch.std(hs, dim=1, correction=ddof)``.  ``window`` / ``hop``
        (frames, window % hop == 0) pool windows instead of the clip -> [B, n_layers, S, n_stats*H];
        a shorter clip of a ragged batch fills its first ``pool_segments(n_samples, window, hop)`` slots, the
        rest are zeros.  ``valid_only`` (Whisper): pool the ceil(n_samples / 320) frames that cover the clip,
        not the 30 s pad.  With all of these at their defaults the call is the plain time-mean above.

        ``frames`` (Whisper audio context): None = the reference's 1500 encoder frames (30 s);
        an int F in [1, 1500] encodes only the first F frames (320 samples each) of every clip -- log-mel,
        convolutions, attention keys and pooling all stop at F; "clip" = the smallest context that covers the
        batch, ``spec.context_frames(L)`` or that of the longest of ``lengths``.  Embeddings at different
        contexts are different features: use one context for training and test."""
        desc = pool_desc(pool, window, hop, ddof, valid_only)
        F = resolve_frames(self.spec, frames, wave.shape[-1] if isinstance(wave, torch.Tensor) else 0, lengths)
        if F is not None or not (desc.stats == _lib.SSE_STAT_MEAN and desc.win == 0 and not desc.valid_only):
            return self._embed_pooled(wave, layer_indices, out, lengths, workspace, check_range, desc, F)
        wave = self._check_wave(wave)
        B, L = wave.shape
        ids = torch.tensor([int(i) for i in layer_indices], dtype=torch.int32)
        n = ids.numel()
        if out is None:
            out = torch.empty((B, n, self.spec.hidden), dtype=torch.float32, device=self.device)
        elif (out.device != self.device or out.dtype != torch.float32 or tuple(out.shape) != (B, n, self.spec.hidden)
              or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous fp32 [{B}, {n}, {self.spec.hidden}] tensor on {self.device}")
        ws = self.workspace(B, L) if workspace is None else workspace
        if ws.numel() < _lib.lib().sse_workspace_bytes(self._h, int(B), int(L)):
            raise ValueError("workspace too small")
        if lengths is None:
            _lib.check(_lib.lib().sse_embed(self._h, wave.data_ptr(), B, L, ids.data_ptr(), n, out.data_ptr(),
                                            ws.data_ptr(), ws.numel(), self._stream()), "sse_embed")
            self._after(check_range)
            return out
        lens = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        if len(lens) != B or min(lens) < 1 or max(lens) > L:
            raise ValueError(f"lengths must be {B} values in [1, {L}]")
        if isinstance(self.spec, WavLMSpec) and min(self.spec.frames(v) for v in lens) <= 0:
            raise _lib.SSEError(-1, "a clip is shorter than the conv receptive field")
        # pinned + non_blocking: the copy is ordered on the current stream without a host sync, so a
        # staged corpus loop keeps its copy / compute overlap (the caching host allocator keeps the
        # pinned buffer alive until the copy has run)
        d_len = torch.tensor(lens, dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)
        _lib.check(_lib.lib().sse_embed_ragged(self._h, wave.data_ptr(), d_len.data_ptr(), B, L, ids.data_ptr(), n,
                                               out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream()),
                   "sse_embed_ragged")
        self._after(check_range)
        return out

    def _embed_pooled(self, wave, layer_indices, out, lengths, workspace, check_range, desc, F=None) -> torch.Tensor:
        wave = self._check_wave(wave)
        B, L = wave.shape
        ids = torch.tensor([int(i) for i in layer_indices], dtype=torch.int32)
        n = ids.numel()
        T = self.output_frames(L, frames=F)
        if T <= 0:
            raise _lib.SSEError(-1, "a clip is shorter than the conv receptive field")
        S = int(_lib.lib().sse_pool_segments(T, desc.win, desc.hop))
        width = _n_stats(desc) * self.spec.hidden
        shape = (B, n, S, width) if desc.win else (B, n, width)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=self.device)
        elif (out.device != self.device or out.dtype != torch.float32 or tuple(out.shape) != shape
              or not out.is_contiguous()):
            raise ValueError(f"out must be a contiguous fp32 {list(shape)} tensor on {self.device}")
        if F is None:
            assert out.numel() == _lib.lib().sse_pool_out_floats(self._h, B, L, n, ctypes.byref(desc))
        else:
            assert out.numel() == _lib.lib().sse_pool_out_floats_ctx(self._h, B, L, F, n, ctypes.byref(desc))
        ws = self.workspace(B, L, frames=F) if workspace is None else workspace
        if ws.numel() < self.workspace_bytes(B, L, frames=F):
            raise ValueError("workspace too small")
        d_len = None
        if lengths is not None:
            lens = [int(v) for v in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
            if len(lens) != B or min(lens) < 1 or max(lens) > L:
                raise ValueError(f"lengths must be {B} values in [1, {L}]")
            if isinstance(self.spec, WavLMSpec) and min(self.spec.frames(v) for v in lens) <= 0:
                raise _lib.SSEError(-1, "a clip is shorter than the conv receptive field")
            d_len = torch.tensor(lens, dtype=torch.int32).pin_memory().to(self.device, non_blocking=True)
        d_len_p = d_len.data_ptr() if d_len is not None else None
        if F is None:
            _lib.check(_lib.lib().sse_embed_pooled(self._h, wave.data_ptr(), d_len_p, B, L, ids.data_ptr(), n,
                                                   ctypes.byref(desc), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                   self._stream()), "sse_embed_pooled")
        else:
            _lib.check(_lib.lib().sse_embed_pooled_ctx(self._h, wave.data_ptr(), d_len_p, B, L, F, ids.data_ptr(), n,
                                                       ctypes.byref(desc), out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                       self._stream()), "sse_embed_pooled_ctx")
        self._after(check_range)
        return out

    def embed_clips(self, clips, layer_indices, **pooling) -> torch.Tensor:
        """A list of 1-D clips of any lengths -> [N, len(layer_indices), H]: one ragged batch
        (zero-padded rows + lengths), every clip embedded at its own length.  ``pooling``: the
        pool / window / hop / ddof / valid_only / frames arguments of ``embed`` (frames="clip": the context
        of the longest clip, shared by the batch)."""
        lens = [int(c.shape[-1]) for c in clips]
        wave = torch.zeros((len(clips), max(lens)), dtype=torch.float32, device=self.device)
        for i, c in enumerate(clips):
            c = c if isinstance(c, torch.Tensor) else torch.from_numpy(np.asarray(c, dtype=np.float32))
            wave[i, :lens[i]] = c.to(self.device, torch.float32)
        return self.embed(wave, layer_indices, lengths=lens, **pooling)

    def hidden_states(self, wave: torch.Tensor, *, frames=None) -> tuple:
        """[B, L] -> tuple of layers+1 tensors [B, T, H] (HF ``output_hidden_states`` semantics).
        ``frames`` (Whisper audio context, see ``embed``): T = F instead of 1500."""
        F = resolve_frames(self.spec, frames, wave.shape[-1] if isinstance(wave, torch.Tensor) else 0)
        wave = self._check_wave(wave)
        B, L = wave.shape
        T = self.output_frames(L, frames=F)
        n_hs = self.spec.layers + 1
        hs = torch.empty((n_hs, B, T, self.spec.hidden), dtype=torch.float32, device=self.device)
        ws = self.workspace(B, L, frames=F)
        if F is None:
            _lib.check(_lib.lib().sse_hidden_states(self._h, wave.data_ptr(), B, L, hs.data_ptr(), ws.data_ptr(),
                                                    ws.numel(), self._stream()), "sse_hidden_states")
        else:
            _lib.check(_lib.lib().sse_hidden_states_ctx(self._h, wave.data_ptr(), B, L, F, hs.data_ptr(), ws.data_ptr(),
                                                        ws.numel(), self._stream()), "sse_hidden_states_ctx")
        self._after()
        return tuple(hs.unbind(0))

    def hidden_states_from_mel(self, mel: torch.Tensor) -> tuple:
        """Whisper only: [B, n_mels, 3000] log-mel -> layers+1 tensors [B, 1500, H]; a log-mel of width 2F
        (``logmel(frames=F)``, or HF input_features[:, :, :2F]) runs the audio context F -> [B, F, H]."""
        if not isinstance(self.spec, WhisperSpec):
            raise TypeError("hidden_states_from_mel is Whisper-only")
        if mel.device != self.device:
            raise ValueError(f"expected a tensor on {self.device}")
        mel = mel.to(torch.float32).contiguous()
        W = mel.shape[2] if mel.dim() == 3 else 0
        if mel.dim() != 3 or mel.shape[1] != self.spec.n_mels or W % 2 or not 2 <= W <= 2 * self.spec.max_positions:
            raise ValueError(f"expected [B, {self.spec.n_mels}, 2F] log-mel with F in [1, {self.spec.max_positions}] "
                             f"({2 * self.spec.max_positions} wide without an audio context), got {tuple(mel.shape)}")
        B = mel.shape[0]
        T = W // 2
        hs = torch.empty((self.spec.layers + 1, B, T, self.spec.hidden), dtype=torch.float32, device=self.device)
        if T == self.spec.max_positions:
            ws = self.workspace(B, self.spec.n_samples)
            _lib.check(_lib.lib().sse_whisper_hidden_states_from_mel(self._h, mel.data_ptr(), B, hs.data_ptr(),
                                                                     ws.data_ptr(), ws.numel(), self._stream()),
                       "sse_whisper_hidden_states_from_mel")
        else:
            ws = self.workspace(B, self.spec.n_samples, frames=T)
            _lib.check(_lib.lib().sse_whisper_hidden_states_from_mel_ctx(self._h, mel.data_ptr(), B, T, hs.data_ptr(),
                                                                         ws.data_ptr(), ws.numel(), self._stream()),
                       "sse_whisper_hidden_states_from_mel_ctx")
        return tuple(hs.unbind(0))


    def whisper_embed(self, wave: torch.Tensor, encoder_indices, decoder_indices, enc_out=None, dec_out=None, *,
                      pool="mean", window=None, hop=None, ddof: int = 1, valid_only: bool = False, frames=None):
        """Whisper: encoder time-means AND 1-token decoder states in one pass
        (REF/whisper_embeddings_large.py:234-299) -> ([B, n_enc, H], [B, n_dec, H]) fp32.
        The pooling arguments (``embed``) apply to the encoder output only (the decoder has one token);
        a non-default pooling runs the encoder statistics and the decoder states as two calls.
        ``frames`` (audio context, see ``embed``): the encoder runs F frames and the decoder cross-attends
        over those F."""
        if not isinstance(self.spec, WhisperSpec):
            raise TypeError("whisper_embed is Whisper-only")
        F = resolve_frames(self.spec, frames, wave.shape[-1] if isinstance(wave, torch.Tensor) else 0)
        if decoder_indices and not self.spec.decoder_layers:
            raise ValueError(f"{self.spec.name} was built without the decoder (decoder_layers=0)")
        desc = pool_desc(pool, window, hop, ddof, valid_only)
        if not (desc.stats == _lib.SSE_STAT_MEAN and desc.win == 0 and not desc.valid_only):
            if len(encoder_indices):
                enc_out = self._embed_pooled(wave, encoder_indices, enc_out, None, None, None, desc, F)
            else:
                enc_out = torch.empty((self._check_wave(wave).shape[0], 0, _n_stats(desc) * self.spec.hidden),
                                      dtype=torch.float32, device=self.device)
            _, dec_out = self.whisper_embed(wave, [], decoder_indices, None, dec_out, frames=F)
            return enc_out, dec_out
        wave = self._check_wave(wave)
        B, L = wave.shape
        H = self.spec.hidden
        eid = torch.tensor([int(i) for i in encoder_indices], dtype=torch.int32)
        did = torch.tensor([int(i) for i in decoder_indices], dtype=torch.int32)
        if enc_out is None:
            enc_out = torch.empty((B, eid.numel(), H), dtype=torch.float32, device=self.device)
        if dec_out is None:
            dec_out = torch.empty((B, did.numel(), H), dtype=torch.float32, device=self.device)
        ws = self.workspace(B, L, frames=F)
        outs = (eid.data_ptr(), eid.numel(), enc_out.data_ptr() if eid.numel() else None, did.data_ptr(), did.numel(),
                dec_out.data_ptr() if did.numel() else None, ws.data_ptr(), ws.numel(), self._stream())
        if F is None:
            _lib.check(_lib.lib().sse_whisper_embed(self._h, wave.data_ptr(), B, L, *outs), "sse_whisper_embed")
        else:
            _lib.check(_lib.lib().sse_whisper_embed_ctx(self._h, wave.data_ptr(), B, L, F, *outs),
                       "sse_whisper_embed_ctx")
        return enc_out, dec_out

    def decoder_hidden_states(self, enc: torch.Tensor) -> tuple:
        """Whisper: ``model.decoder(input_ids=zeros([B, 1]), encoder_hidden_states=enc)`` hidden states:
        enc [B, 1500, H] -> decoder_layers+1 tensors [B, 1, H] fp32; enc [B, F, H] (the last state of an
        audio context F) cross-attends over those F frames."""
        if not isinstance(self.spec, WhisperSpec) or not self.spec.decoder_layers:
            raise TypeError("decoder_hidden_states needs a Whisper spec with decoder_layers > 0")
        H = self.spec.hidden
        if (enc.device != self.device or enc.dim() != 3 or enc.shape[2] != H
                or not 1 <= enc.shape[1] <= self.spec.max_positions):
            raise ValueError(f"expected [B, F <= {self.spec.max_positions}, {H}] encoder states on {self.device}, "
                             f"got {tuple(enc.shape)}")
        T = enc.shape[1]
        enc = enc.to(torch.float32).contiguous()
        B = enc.shape[0]
        hs = torch.empty((self.spec.decoder_layers + 1, B, 1, H), dtype=torch.float32, device=self.device)
        if T == self.spec.max_positions:
            ws = self.workspace(B, self.spec.n_samples)
            _lib.check(_lib.lib().sse_whisper_decoder_hidden_states(self._h, enc.data_ptr(), B, hs.data_ptr(),
                                                                    ws.data_ptr(), ws.numel(), self._stream()),
                       "sse_whisper_decoder_hidden_states")
        else:
            ws = self.workspace(B, self.spec.n_samples, frames=T)
            _lib.check(_lib.lib().sse_whisper_decoder_hidden_states_ctx(self._h, enc.data_ptr(), B, T, hs.data_ptr(),
                                                                        ws.data_ptr(), ws.numel(), self._stream()),
                       "sse_whisper_decoder_hidden_states_ctx")
        return tuple(hs.unbind(0))


_LOGMEL_SPEC = WhisperSpec()   # the log-mel's frame arithmetic is the same for every Whisper (1500 frames of 320)


def logmel(wave: torch.Tensor, n_mels: int = 80, *, frames=None) -> torch.Tensor:
    """Whisper log-mel on device: [B, L] (L <= 480000) -> [B, n_mels, 3000] (HF layout).  ``frames`` (audio
    context F, an int or "clip"): the log-mel of each clip cut at 320 F samples, mel frames [0, 2F) ->
    [B, n_mels, 2F], the per-clip max of the -8 clamp over those frames."""
    F = resolve_frames(_LOGMEL_SPEC, frames, wave.shape[-1])
    if wave.dim() == 1:
        wave = wave[None]
    wave = wave.to(torch.float32).contiguous()
    B, L = wave.shape
    L_ = _lib.lib()
    stream = ctypes.c_void_p(torch.cuda.current_stream(wave.device).cuda_stream)
    if F is not None:
        n = L_.sse_logmel_workspace_bytes_ctx(B, n_mels, F)
        ws = torch.empty(n, dtype=torch.uint8, device=wave.device)
        out = torch.empty((B, n_mels, 2 * F), dtype=torch.float32, device=wave.device)
        _lib.check(L_.sse_logmel_ctx(wave.data_ptr(), B, L, n_mels, F, out.data_ptr(), ws.data_ptr(), n, stream),
                   "sse_logmel_ctx")
        return out
    n = L_.sse_logmel_workspace_bytes(B, n_mels)
    ws = torch.empty(n, dtype=torch.uint8, device=wave.device)
    out = torch.empty((B, n_mels, 3000), dtype=torch.float32, device=wave.device)
    _lib.check(L_.sse_logmel(wave.data_ptr(), B, L, n_mels, out.data_ptr(), ws.data_ptr(), n, stream), "sse_logmel")
    return out


def pool_states(x: torch.Tensor, lengths=None, pool="mean", window=None, hop=None, ddof: int = 1) -> torch.Tensor:
    """The statistics-pooling kernel on its own (sse_pool): x [B, T, H] fp32 / bf16 / fp16 on the GPU, H % 4 == 0,
    optional per-clip frame counts ``lengths`` -> [B, n_stats*H], or [B, S, n_stats*H] with ``window`` / ``hop``
    (the arguments of ``SSEModel.embed``)."""
    desc = pool_desc(pool, window, hop, ddof)
    dts = {torch.float32: _lib.SSE_DTYPE_F32, torch.bfloat16: _lib.SSE_DTYPE_BF16, torch.float16: _lib.SSE_DTYPE_FP16}
    if x.dim() != 3 or x.dtype not in dts or not x.is_cuda:
        raise TypeError("x must be a [B, T, H] fp32 / bf16 / fp16 tensor on the GPU")
    x = x.contiguous()
    B, T, H = x.shape
    S = int(_lib.lib().sse_pool_segments(T, desc.win, desc.hop))
    width = _n_stats(desc) * H
    out = torch.empty((B, S, width) if desc.win else (B, width), dtype=torch.float32, device=x.device)
    d_len = None
    if lengths is not None:
        d_len = torch.as_tensor(lengths, dtype=torch.int32).to(x.device)
        if d_len.numel() != B:
            raise ValueError(f"lengths must hold {B} frame counts")
    _lib.check(_lib.lib().sse_pool(dts[x.dtype], x.data_ptr(), d_len.data_ptr() if d_len is not None else None, B, T, H,
                                   ctypes.byref(desc), out.data_ptr(),
                                   ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)), "sse_pool")
    return out


def normalize(wave: torch.Tensor) -> torch.Tensor:
    """Wav2Vec2FeatureExtractor(do_normalize=True) on device: per-clip zero mean / unit variance."""
    if wave.dim() == 1:
        wave = wave[None]
    wave = wave.to(torch.float32).contiguous()
    B, L = wave.shape
    ws = torch.empty(8 * B, dtype=torch.uint8, device=wave.device)
    out = torch.empty_like(wave)
    _lib.check(_lib.lib().sse_normalize(wave.data_ptr(), B, L, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                        ctypes.c_void_p(torch.cuda.current_stream(wave.device).cuda_stream)),
               "sse_normalize")
    return out


_ZERO = {}


def gemm(a: torch.Tensor, b: torch.Tensor, bias=None, resid=None, act: str | None = None,
         out_dtype=torch.float32) -> torch.Tensor:
    """The path's MFMA GEMM on its own: a [M, K] @ b[N, K]^T (+bias) (gelu) (+resid).
    a, b both bf16 (bf16 MFMA) or both fp32 (exact-f32 MFMA).  act: None | "gelu" (erf form) |
    "gelu_fast" (the bf16 path's gelu_fast2 epilogue, common.h)."""
    if a.dtype != b.dtype or a.dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("a and b must both be bf16 or both fp32")
    M, K = a.shape
    N = b.shape[0]
    dev = a.device
    z = _ZERO.get(dev)
    if z is None:
        z = _ZERO[dev] = torch.zeros(64, dtype=torch.float32, device=dev)
    a, b = a.contiguous(), b.contiguous()
    cf = torch.empty((M, N), dtype=torch.float32, device=dev) if out_dtype == torch.float32 else None
    ct = torch.empty((M, N), dtype=a.dtype, device=dev) if out_dtype != torch.float32 else None
    dt = _lib.SSE_DTYPE_BF16 if a.dtype == torch.bfloat16 else _lib.SSE_DTYPE_F32
    bias_p = bias.contiguous().data_ptr() if bias is not None else None
    res_p = resid.contiguous().data_ptr() if resid is not None else None
    _lib.check(_lib.lib().sse_gemm(dt, a.data_ptr(), b.data_ptr(), bias_p, res_p,
                                   cf.data_ptr() if cf is not None else None,
                                   ct.data_ptr() if ct is not None else None, M, N, K, {None: 0, "gelu": 1, "gelu_fast": 2}[act],
                                   z.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)),
               "sse_gemm")
    return cf if cf is not None else ct


def mx_scale_bytes(R: int, K: int) -> int:
    return int(_lib.lib().sse_mx_scale_bytes(R, K))


def mx_quantize(x: torch.Tensor, role: int = 0) -> tuple[torch.Tensor, torch.Tensor]:
    """MX-fp8 quantisation on the GPU: fp32 x [R, K] (K % 128 == 0) -> (e4m3 bytes uint8 [R, K],
    E8M0 scales uint8 in the GEMM's role-0 (A) / role-1 (B) tile layout)."""
    x = x.contiguous()
    R, K = x.shape
    q = torch.empty((R, K), dtype=torch.uint8, device=x.device)
    sc = torch.empty(mx_scale_bytes(R, K), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.lib().sse_mx_quantize(x.data_ptr(), R, K, role, q.data_ptr(), sc.data_ptr(),
                                          ctypes.c_void_p(torch.cuda.current_stream(x.device).cuda_stream)),
               "sse_mx_quantize")
    return q, sc


def mx_quantize_host(x: np.ndarray, role: int = 0) -> tuple[np.ndarray, np.ndarray]:
    """The host quantiser libsse.so applies to weights at sse_model_create (no GPU needed)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    R, K = x.shape
    q = np.empty((R, K), dtype=np.uint8)
    sc = np.empty(mx_scale_bytes(R, K), dtype=np.uint8)
    _lib.check(_lib.lib().sse_mx_quantize_host(x.ctypes.data, R, K, role, q.ctypes.data, sc.ctypes.data),
               "sse_mx_quantize_host")
    return q, sc


def gemm_mx(a_q: torch.Tensor, a_s: torch.Tensor, b_q: torch.Tensor, b_s: torch.Tensor, bias=None, resid=None,
            act: str | None = None, out: str = "fp32"):
    """MX-fp8 GEMM: dequant(a) [M, K] @ dequant(b)[N, K]^T (+bias) (gelu) (+resid).  out: "fp32",
    "bf16" or "fp8" (returns (e4m3 [M, N], scales in the A layout of a GEMM with K = N))."""
    M, K = a_q.shape
    N = b_q.shape[0]
    dev = a_q.device
    cf = torch.empty((M, N), dtype=torch.float32, device=dev) if out == "fp32" else None
    ct = None
    cs = None
    if out == "bf16":
        ct = torch.empty((M, N), dtype=torch.bfloat16, device=dev)
    elif out == "fp8":
        ct = torch.empty((M, N), dtype=torch.uint8, device=dev)
        cs = torch.empty(mx_scale_bytes(M, N), dtype=torch.uint8, device=dev)
    bias_p = bias.contiguous().data_ptr() if bias is not None else None
    res_p = resid.contiguous().data_ptr() if resid is not None else None
    _lib.check(_lib.lib().sse_gemm_mx(a_q.data_ptr(), a_s.data_ptr(), b_q.data_ptr(), b_s.data_ptr(), bias_p, res_p,
                                      cf.data_ptr() if cf is not None else None,
                                      ct.data_ptr() if ct is not None else None,
                                      cs.data_ptr() if cs is not None else None, M, N, K,
                                      {None: 0, "gelu": 1, "gelu_fast": 2}[act],
                                      ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "sse_gemm_mx")
    if out == "fp32":
        return cf
    return (ct, cs) if out == "fp8" else ct
