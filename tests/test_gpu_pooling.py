"""Statistics / windowed pooling on the GPU (pool_stats_kernel, sse_pool, sse_embed_pooled).

The reference is always torch in fp64 on the host, applied to the same fp32 values the kernel pools: the
input of the kernel hook, or ``hidden_states()`` of the same model and dtype.  Bars: max is bit-equal to the
fp32 maximum; mean and std are within 1e-5 * max|ref| per output vector (identical fp32 inputs, fp64
accumulation: only the final rounding, ~6e-8, is left; a single-precision sum of squares on data offset by
100 misses it by ~1e-3); absent segments and empty clips are exactly 0 and nothing is NaN."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MASKS = [1, 2, 3, 4, 5, 6, 7]
NAMES = {1: "mean", 2: "std", 4: "max"}
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _pool_arg(mask):
    return tuple(NAMES[b] for b in (1, 2, 4) if mask & b)


def _segments(T, win, hop):
    if win == 0 or T <= win:
        return 1
    return 1 + -(-(T - win) // hop)


def _ref_clip(h, win, hop):
    """h [T, H] fp64 on the host -> {"mean", "std0", "std1", "max"} [S(T), H] fp64 (T >= 1)."""
    T = h.shape[0]
    S = _segments(T, win, hop)
    segs = [h] if S == 1 else [h[s * hop:min(s * hop + win, T)] for s in range(S)]
    if S > 1:   # the full windows in one strided view, the (shorter) tail apart
        nfull = (T - win) // hop + 1
        u = h.unfold(0, win, hop)[:nfull]                    # [nfull, H, win]
        tail = segs[nfull:]
        assert len(tail) <= 1
        cat = lambda a, f: torch.cat([a] + [f(t)[None] for t in tail])   # noqa: E731
        return {"mean": cat(u.mean(-1), lambda t: t.mean(0)),
                "std0": cat(u.std(-1, correction=0), lambda t: t.std(0, correction=0)),
                "std1": cat(u.std(-1, correction=1) if win > 1 else torch.zeros_like(u[..., 0]),
                            lambda t: t.std(0, correction=1) if t.shape[0] > 1 else torch.zeros_like(t[0])),
                "max": cat(u.amax(-1), lambda t: t.amax(0))}
    return {"mean": h.mean(0)[None], "std0": h.std(0, correction=0)[None],
            "std1": (h.std(0, correction=1) if T > 1 else torch.zeros_like(h[0]))[None], "max": h.amax(0)[None]}


def _ref_batch(hs, tlens, win, hop, slots):
    """hs: list of [T_b, H] fp64 host tensors (already cut to each clip's frames) -> per statistic
    [B, slots, H] with zeros in the absent slots, and the list of segment counts."""
    H = hs[0].shape[-1]
    out = {k: torch.zeros((len(hs), slots, H), dtype=torch.float64) for k in ("mean", "std0", "std1", "max")}
    counts = []
    for b, h in enumerate(hs):
        if h.shape[0] == 0:
            counts.append(0)
            continue
        r = _ref_clip(h, win, hop)
        S = r["mean"].shape[0]
        assert S == _segments(h.shape[0], win, hop) <= slots
        counts.append(S)
        for k in out:
            out[k][b, :S] = r[k]
    return out, counts


def _check(got, ref, counts, mask, ddof, what, max_exact=True):
    """got [B, slots, n_stats*H] (host fp32) against the reference of _ref_batch."""
    B, slots, W = got.shape
    H = ref["mean"].shape[-1]
    assert W == bin(mask).count("1") * H, what
    assert not torch.isnan(got).any(), what
    k = 0
    for bit, key in ((1, "mean"), (2, f"std{ddof}"), (4, "max")):
        if not mask & bit:
            continue
        g = got[:, :, k * H:(k + 1) * H].double()
        r = ref[key]
        k += 1
        for b, S in enumerate(counts):
            assert (g[b, S:] == 0).all(), (what, key, b, "absent segments must be zeros")
        if bit == 4 and max_exact:
            assert torch.equal(g, r), (what, key)
            continue
        err = (g - r).abs().amax(-1)
        bar = 1e-5 * r.abs().amax(-1)
        assert (err <= bar).all(), (what, key, float((err - bar).max()), float(err.max()), float(r.abs().max()))


def _data(B, T, H, dtype, seed):
    """Per-column offset of 100 and unit spread (a single-precision sum of squares fails the std bar)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((B, T, H), generator=g) + 100.0 + torch.randn((1, 1, H), generator=g)
    return x.to(TORCH_DT[dtype]).cuda()


def _windows(T):
    return [(0, 0), (4, 4), (8, 2), (50, 25), (T, T), (T + 5, 1)]


@pytest.mark.parametrize("T", [1, 2, 17, 149, 1030, 1500])   # 1030 > POOL_TMAX = 1024
@pytest.mark.parametrize("dtype", ["f32", "bf16", "fp16"])
def test_pool_kernel_matches_fp64(dtype, T):
    """sse_pool: every statistic mask, ddof, window and ragged frame-count pattern; H = 260 has a partial
    256-column block, the padding rows hold large garbage."""
    from ssr_amd.model import pool_states
    B = 3
    for H in (4, 260, 768):
        x = _data(B, T, H, dtype, seed=T * 7 + H)
        for tl in (None, [T, 1, 0], [T, T - 1, (T + 1) // 2]):
            xg = x
            if tl is not None:
                xg = x.clone()
                g = torch.Generator().manual_seed(5)
                for b, n in enumerate(tl):
                    xg[b, n:] = (torch.randn((T - n, H), generator=g) * 1e4).to(x.dtype).cuda()
            host = xg.float().double().cpu()
            hs = [host[b, :(T if tl is None else tl[b])] for b in range(B)]
            for win, hop in _windows(T):
                slots = _segments(T, win, hop)
                ref, counts = _ref_batch(hs, tl, win, hop, slots)
                for ddof in (0, 1):
                    for mask in MASKS:
                        got = pool_states(xg, tl, _pool_arg(mask), win or None, hop or None, ddof)
                        got = got.cpu().reshape(B, slots, -1)
                        _check(got, ref, counts, mask, ddof, (dtype, T, H, tl, win, hop, ddof, mask))


def test_pool_kernel_window_wider_than_the_ring():
    """win / hop at and past the kernel's 8 LDS slots: a full ring (one new chunk per round), and the
    per-segment form for more chunk partials than slots."""
    from ssr_amd.model import pool_states
    B, T, H = 2, 149, 260
    x = _data(B, T, H, "f32", seed=9)
    tl = [T, 77]
    host = x.double().cpu()
    hs = [host[b, :tl[b]] for b in range(B)]
    for win, hop in ((14, 2), (16, 2), (24, 3), (18, 2), (34, 2), (40, 1), (64, 4), (60, 3)):
        slots = _segments(T, win, hop)
        ref, counts = _ref_batch(hs, tl, win, hop, slots)
        got = pool_states(x, tl, "mean_std_max", win, hop).cpu()
        _check(got, ref, counts, 7, 1, (win, hop))


# ------------------------------------------------------------------------------------------------
# model level
_MODELS = {}


def _wavlm(wavlm_sd, dtype):
    from ssr_amd import config as C
    from ssr_amd.model import SSEModel
    if ("wavlm", dtype) not in _MODELS:
        _MODELS[("wavlm", dtype)] = SSEModel(C.WAVLM_BASE, wavlm_sd, device="cuda:0", dtype=dtype)
    return _MODELS[("wavlm", dtype)]


def _whisper(dtype):
    from ssr_amd import config as C, synth
    from ssr_amd.model import SSEModel
    if ("whisper", dtype) not in _MODELS:
        _MODELS[("whisper", dtype)] = SSEModel(C.WHISPER_TINY, synth.synth_whisper_state_dict(C.WHISPER_TINY, seed=11),
                                               device="cuda:0", dtype=dtype)
    return _MODELS[("whisper", dtype)]


def _ragged_batch(lens, seed, garbage=True):
    from ssr_amd import synth
    L = max(lens)
    rng = np.random.default_rng(seed)
    wave = (rng.standard_normal((len(lens), L)).astype(np.float32) * 3.0) if garbage else np.zeros((len(lens), L), np.float32)
    clips = [synth.synth_clips(1, n, seed=seed + i)[0] for i, n in enumerate(lens)]
    for i, c in enumerate(clips):
        wave[i, :len(c)] = c
    return torch.from_numpy(wave).cuda(), clips


def _check_layers(got, hs_per_clip, idx, folded, win, hop, what):
    """got [B, n_layers, (S,) 3H] of pool="mean_std_max"; hs_per_clip[b][layer] = [T_b, H] fp64 host."""
    B, n = got.shape[:2]
    got = got.cpu().reshape(B, n, -1, got.shape[-1])
    slots = got.shape[2]
    for j, layer in enumerate(idx):
        ref, counts = _ref_batch([h[layer] for h in hs_per_clip], None, win, hop, slots)
        _check(got[:, j], ref, counts, 7, 1, (what, layer), max_exact=layer not in folded)


def _folded(dtype, layers):
    """WavLM-base bf16 / fp16: the post-LN of layers 1..12 is folded into the pooling (Sink::emit_ln), so the
    pooled elements are normalised in-kernel: max within the mean / std bar instead of bit-equal."""
    return set(range(1, layers + 1)) if dtype in ("bf16", "fp16") else set()


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16", "fp16x3"])
def test_wavlm_pooled_matches_hidden_states(wavlm_sd, dtype):
    from ssr_amd import synth
    m = _wavlm(wavlm_sd, dtype)
    idx = [12, 11, 6, 0]
    folded = _folded(dtype, 12)
    wave = torch.from_numpy(synth.synth_clips(6, 16000, seed=21)).cuda()
    hs = [h.double().cpu() for h in m.hidden_states(wave)]
    per_clip = [[h[b] for h in hs] for b in range(6)]
    full = m.embed(wave, idx, pool="mean_std_max")
    assert tuple(full.shape) == (6, 4, 3 * 768)
    _check_layers(full, per_clip, idx, folded, 0, 0, (dtype, "full"))
    wind = m.embed(wave, idx, pool="mean_std_max", window=50, hop=25)   # 49 frames: one segment
    assert tuple(wind.shape) == (6, 4, 1, 3 * 768)
    _check_layers(wind, per_clip, idx, folded, 50, 25, (dtype, "window"))
    # the mean slot against today's embed()
    base = m.embed(wave, idx)
    ms = m.embed(wave, idx, pool="mean_std")
    assert tuple(ms.shape) == (6, 4, 2 * 768)
    err = (ms[..., :768] - base).abs().amax(-1)
    assert (err <= 1e-6 * base.abs().amax(-1)).all(), float(err.max())
    assert torch.equal(ms[..., 768:], full[..., 768:2 * 768])


@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16", "fp16x3"])
def test_wavlm_pooled_ragged(wavlm_sd, dtype):
    """One ragged batch (149, 1, 38 and 93 frames): fp64 pooling of each clip's own hidden states, and every
    clip bit-equal to that clip pooled alone."""
    m = _wavlm(wavlm_sd, dtype)
    idx = [12, 11, 6, 0]
    lens = [48000, 400, 12345, 30000]
    wave, clips = _ragged_batch(lens, 300)
    per_clip = [[h[0].double().cpu() for h in m.hidden_states(torch.from_numpy(c).cuda()[None])] for c in clips]
    assert [h[0].shape[0] for h in per_clip] == [149, 1, 38, 93]
    for kw, win, hop in ((dict(), 0, 0), (dict(window=50, hop=25), 50, 25)):
        got = m.embed(wave, idx, lengths=lens, pool="mean_std_max", **kw)
        _check_layers(got, per_clip, idx, _folded(dtype, 12), win, hop, (dtype, kw))
        for i, c in enumerate(clips):
            one = m.embed(torch.from_numpy(c).cuda()[None], idx, pool="mean_std_max", **kw)
            S = one.shape[2] if kw else None
            assert torch.equal(got[i:i + 1, :, :S] if kw else got[i:i + 1], one), (dtype, kw, i)
            if kw:
                assert S == m.pool_segments(lens[i], 50, 25) and (got[i, :, S:] == 0).all()


def test_wavlm_pooled_half_batch_split(wavlm_sd):
    """B = 128 is the smallest batch split_applies takes (SPLIT_MIN): the two half-batches write their own
    rows of the [B][n_layers][S][n_stats*H] output.  Rows on both sides of the split against fp64 pooling of
    hidden_states() of those clips, and bit-equal to the same clips in an unsplit batch."""
    from ssr_amd import synth
    m = _wavlm(wavlm_sd, "bf16")
    idx = [12, 11, 6, 0]
    wave = torch.from_numpy(synth.synth_clips(128, 16000, seed=33)).cuda()
    rows = [0, 1, 63, 64, 65, 127]
    hs = [h.double().cpu() for h in m.hidden_states(wave[rows])]
    per_clip = [[h[b] for h in hs] for b in range(len(rows))]
    for kw, win, hop in ((dict(), 0, 0), (dict(window=16, hop=8), 16, 8)):
        got = m.embed(wave, idx, pool="mean_std_max", **kw)
        _check_layers(got[rows], per_clip, idx, _folded("bf16", 12), win, hop, ("split", kw))
        assert torch.equal(got[rows], m.embed(wave[rows], idx, pool="mean_std_max", **kw))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_whisper_pooled_and_valid_only(dtype):
    from ssr_amd import config as C
    m = _whisper(dtype)
    nl = C.WHISPER_TINY.layers
    idx = [nl, nl - 1, nl // 2, 0]
    lens = [16000, 48000, 7000]
    wave, _ = _ragged_batch(lens, 5, garbage=False)   # Whisper pads each clip with zeros to 30 s
    hs = [h.double().cpu() for h in m.hidden_states(wave)]
    valid = [-(-n // 320) for n in lens]
    assert valid == [50, 150, 22]
    for kw, win, hop in ((dict(), 0, 0), (dict(window=50, hop=25), 50, 25)):
        got = m.embed(wave, idx, lengths=lens, pool="mean_std_max", valid_only=True, **kw)
        _check_layers(got, [[h[b, :valid[b]] for h in hs] for b in range(3)], idx, set(), win, hop, (dtype, "valid", kw))
        if kw:
            for b, n in enumerate(lens):
                assert m.pool_segments(n, 50, 25, valid_only=True) == _segments(valid[b], 50, 25)
        got = m.embed(wave, idx, lengths=lens, pool="mean_std_max", valid_only=False, **kw)
        _check_layers(got, [[h[b] for h in hs] for b in range(3)], idx, set(), win, hop, (dtype, "all", kw))
    # valid_only without lengths: the row length counts for every clip
    got = m.embed(wave[:, :16000], idx, pool="mean_std_max", valid_only=True)
    hs16 = [h.double().cpu() for h in m.hidden_states(wave[:, :16000])]
    _check_layers(got, [[h[b, :50] for h in hs16] for b in range(3)], idx, set(), 0, 0, (dtype, "valid, no lengths"))
    # the default whisper_embed call is today's; its pooling applies to the encoder output only
    dec = [0, C.WHISPER_TINY.decoder_layers] if C.WHISPER_TINY.decoder_layers else []
    e0, d0 = m.whisper_embed(wave, idx, dec)
    e1, d1 = m.whisper_embed(wave, idx, dec, pool="mean")
    assert torch.equal(e0, e1) and torch.equal(d0, d1) and torch.equal(e0, m.embed(wave, idx))
    e2, d2 = m.whisper_embed(wave, idx, dec, pool="mean_std")
    assert torch.equal(e2, m.embed(wave, idx, pool="mean_std")) and torch.equal(d2, d0)


@pytest.mark.parametrize("kind", ["wavlm", "whisper"])
def test_default_pooling_is_unchanged(wavlm_sd, kind):
    from ssr_amd import synth
    m = _wavlm(wavlm_sd, "bf16") if kind == "wavlm" else _whisper("bf16")
    idx = [m.spec.layers, 1, 0]
    wave = torch.from_numpy(synth.synth_clips(3, 16000, seed=2)).cuda()
    a = m.embed(wave, idx)
    assert torch.equal(a, m.embed(wave, idx, pool="mean"))
    assert torch.equal(a, m.embed(wave, idx, pool=("mean",), ddof=0))
    lens = [16000, 9000, 4000]
    assert torch.equal(m.embed(wave, idx, lengths=lens), m.embed(wave, idx, lengths=lens, pool="mean"))


# ------------------------------------------------------------------------------------------------
# C-ABI
def _call_pooled(m, wave, lens, ids, desc, out, ws_bytes=None):
    from ssr_amd import _lib
    B, L = wave.shape
    ws = m.workspace(B, L)
    return _lib.lib().sse_embed_pooled(m._h, wave.data_ptr(), lens.data_ptr() if lens is not None else None, B, L,
                                       ids.data_ptr(), ids.numel(), ctypes.byref(desc) if desc is not None else None,
                                       out.data_ptr(), ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes,
                                       m._stream())


def test_c_abi_rejects_invalid_descriptors(wavlm_sd):
    from ssr_amd import _lib, synth
    m = _wavlm(wavlm_sd, "bf16")
    wave = torch.from_numpy(synth.synth_clips(2, 16000, seed=4)).cuda()
    ids = torch.tensor([12, 0], dtype=torch.int32)
    out = torch.full((2, 2, 49, 3 * 768), 1234.5, device="cuda")
    D = _lib.sse_pool_desc
    bad = [D(0, 1, 0, 0, 0), D(8, 1, 0, 0, 0), D(1 | 16, 1, 0, 0, 0), D(-1, 1, 0, 0, 0), D(3, 2, 0, 0, 0),
           D(3, -1, 0, 0, 0), D(3, 1, -4, 2, 0), D(3, 1, 8, 0, 0), D(3, 1, 8, -2, 0), D(3, 1, 8, 3, 0), None]
    for d in bad:
        assert _call_pooled(m, wave, None, ids, d, out) == _lib.SSE_ERR_INVALID, d and tuple(getattr(d, f) for f, _ in d._fields_)
        assert _lib.lib().sse_pool_out_floats(m._h, 2, 16000, 2, ctypes.byref(d) if d is not None else None) == 0
        if d is not None:
            x = torch.zeros((1, 4, 8), device="cuda")
            assert _lib.lib().sse_pool(0, x.data_ptr(), None, 1, 4, 8, ctypes.byref(d), out.data_ptr(), None) == _lib.SSE_ERR_INVALID
    torch.cuda.synchronize()
    assert (out == 1234.5).all()
    good = D(3, 1, 8, 2, 0)
    assert _lib.lib().sse_pool_out_floats(m._h, 2, 16000, 2, ctypes.byref(good)) == 2 * 2 * _segments(49, 8, 2) * 2 * 768
    assert _call_pooled(m, wave, None, ids, good, out, ws_bytes=1024) == _lib.SSE_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert (out == 1234.5).all()
    assert _call_pooled(m, wave, None, ids, good, out) == 0
    torch.cuda.synchronize()
    n = 2 * 2 * _segments(49, 8, 2) * 2 * 768
    assert torch.isfinite(out.flatten()[:n]).all() and (out.flatten()[n:] == 1234.5).all()


def test_c_abi_clamps_out_of_range_lengths(wavlm_sd):
    """Past the Python wrapper's checks: a length beyond the row counts as the row, one under the receptive
    field and a negative one pool to zeros; nothing is read outside a clip's rows."""
    from ssr_amd import _lib, synth
    m = _wavlm(wavlm_sd, "bf16")
    L = 48000
    wave = torch.from_numpy(synth.synth_clips(4, L, seed=41)).cuda()
    lens = torch.tensor([L, 10 * L, 200, -5], dtype=torch.int32, device="cuda")
    ids = torch.tensor([12, 6, 0], dtype=torch.int32)
    desc = _lib.sse_pool_desc(7, 1, 50, 25, 0)
    S = _segments(149, 50, 25)
    out = torch.full((4, 3, S, 3 * 768), float("nan"), device="cuda")
    assert _call_pooled(m, wave, lens, ids, desc, out) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    full = m.embed(wave[:2], [12, 6, 0], pool="mean_std_max", window=50, hop=25)
    assert torch.equal(out[:2], full)
    assert (out[2:] == 0).all()
    # Whisper valid-frame counts are clamped the same way
    w = _whisper("fp32")
    wv = wave[:3, :32000].contiguous()
    lw = torch.tensor([10 * 32000, -5, 16000], dtype=torch.int32, device="cuda")
    wid = torch.tensor([w.spec.layers, 0], dtype=torch.int32)
    d2 = _lib.sse_pool_desc(7, 1, 0, 0, 1)
    o2 = torch.full((3, 2, 3 * w.spec.hidden), float("nan"), device="cuda")
    assert _call_pooled(w, wv, lw, wid, d2, o2) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(o2).all() and (o2[1] == 0).all()
    ref = wv.clone()
    ref[2, 16000:].zero_()
    r2 = w.embed(ref, [w.spec.layers, 0], lengths=[32000, 1, 16000], pool="mean_std_max", valid_only=True)
    assert torch.equal(o2[0], r2[0]) and torch.equal(o2[2], r2[2])


# ------------------------------------------------------------------------------------------------
# drop-in functions
def test_extract_wavlm_pooling_keyword(wavlm_sd):
    from ssr_amd import config as C, synth
    from ssr_amd.extract import extract_embeddings_from_audio_wavlm
    from ssr_amd.hf import Wav2Vec2FeatureExtractor, WavLMModel
    model = WavLMModel(_wavlm(wavlm_sd, "fp32"))
    fe = Wav2Vec2FeatureExtractor(do_normalize=False, device="cuda:0")
    clip = synth.synth_clips(1, 20000, seed=8)[0]
    layers = [12, 6, 0]
    base = extract_embeddings_from_audio_wavlm(clip, model, fe, "cuda:0", layers)
    got = extract_embeddings_from_audio_wavlm(clip, model, fe, "cuda:0", layers, pooling="mean_std")
    assert sorted(got) == sorted(base) == ["layer_0", "layer_12", "layer_6"]

    class Generic:   # not a WavLMModel: the hidden-states route through _pool_generic
        def __call__(self, *a, **k):
            return model(*a, **k)

    gen = extract_embeddings_from_audio_wavlm(clip, Generic(), fe, "cuda:0", layers, pooling="mean_std")
    H = C.WAVLM_BASE.hidden
    for k in base:
        assert got[k].dtype == np.float32 and got[k].shape == (2 * H,)
        assert np.abs(got[k][:H] - base[k]).max() <= 1e-6 * np.abs(base[k]).max()
        for part in (slice(0, H), slice(H, 2 * H)):
            # the generic route pools in fp32 with torch: its own rounding (a few 6e-8 steps) is inside the 1e-5 bar
            assert np.abs(got[k][part] - gen[k][part]).max() <= 1e-5 * np.abs(gen[k][part]).max(), k
    with pytest.raises(ValueError):
        extract_embeddings_from_audio_wavlm(clip, model, fe, "cuda:0", layers, pooling="median")
