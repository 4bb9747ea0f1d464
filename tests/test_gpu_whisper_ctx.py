"""Whisper audio context on the GPU (``frames=F``: encode only the first F encoder frames of every clip).

References are the numpy oracle on the CPU, fed the definition's own input: ``log_mel(w[:320 F])[:, :2F]`` and
``WhisperOracle.hidden_states`` of that mel (it slices embed_positions to the mel's width).  Bars are the
project's, from tests/test_gpu_whisper.py: log-mel max abs 2e-4; fp32 and fp16x3 rel-L2 <= 1e-4; bf16 rel-L2 <=
3e-2 and cosine >= 0.999; fp8 rel-L2 <= 0.08 and cosine >= 0.995.  Everything that must not change is bit-exact:
frames=1500 against the call without a context, a clip alone against the clip in a batch, "clip" against the
integer it resolves to."""
import ctypes

import numpy as np
import pytest
import torch

from test_gpu_pooling import _check, _ref_batch, _segments

pytestmark = pytest.mark.gpu

BARS = {"fp32": (1e-4, 0.9999999), "fp16x3": (1e-4, 0.9999999), "bf16": (3e-2, 0.999), "fp8": (0.08, 0.995)}
_MODELS, _ORACLES, _REFS = {}, {}, {}


def _spec(name):
    from ssr_amd import config as C
    return {"tiny": C.WHISPER_TINY, "tiny_dec": C.WHISPER_TINY_DEC, "small": C.WHISPER_SMALL}[name]


def _sd(name):
    from ssr_amd import synth
    if name not in _ORACLES:
        from oracle.whisper import WhisperOracle
        sd = synth.synth_whisper_state_dict(_spec(name), seed=11)
        _ORACLES[name] = (sd, WhisperOracle(_spec(name), sd))
    return _ORACLES[name]


def _model(name, dtype):
    from ssr_amd.model import SSEModel
    if (name, dtype) not in _MODELS:
        _MODELS[(name, dtype)] = SSEModel(_spec(name), _sd(name)[0], device="cuda:0", dtype=dtype)
    return _MODELS[(name, dtype)]


def _batch(lens, seed):
    """Clips of the given lengths as zero-padded rows of one [B, max(lens)] batch (Whisper's own padding)."""
    from ssr_amd import synth
    clips = [synth.synth_clips(1, n, seed=seed + i)[0] for i, n in enumerate(lens)]
    wave = np.zeros((len(lens), max(lens)), np.float32)
    for i, c in enumerate(clips):
        wave[i, :len(c)] = c
    return wave


def _ctx_mel(w, F, n_mels=80):
    from oracle.whisper import log_mel
    return log_mel(w[:F * 320], n_mels)[:, :2 * F]


def _ref_states(name, wave, F, key):
    """Oracle hidden states of every clip at context F, [B][layers+1][F, D], computed once per (model, batch, F)."""
    k = (name, key, F)
    if k not in _REFS:
        o = _sd(name)[1]
        _REFS[k] = [np.stack(o.hidden_states(_ctx_mel(w, F))) for w in wave]
    return _REFS[k]


def _rel(a, b):
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


def _cos(a, b):
    return (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def _lens(F):
    """A 1 s clip, a 3 s clip and a clip longer than the context."""
    return [16000, 48000, max(48000, F * 320) + 777]


# ------------------------------------------------------------------------------------------------
# 1. log-mel
@pytest.mark.parametrize("v1", [0, 1])
@pytest.mark.parametrize("n_mels", [80, 128])
@pytest.mark.parametrize("F", [1, 10, 37, 150, 1500])
def test_logmel_context(F, n_mels, v1):
    from ssr_amd import _lib
    from ssr_amd.model import logmel
    wave = _batch([1000, F * 320, F * 320 + 777], seed=100 + F)
    w = torch.from_numpy(wave).cuda()
    with _lib.option("logmel_v1", v1):
        got = logmel(w, n_mels, frames=F)
        full = logmel(w, n_mels) if F == 1500 else None
        z = logmel(torch.zeros((1, 16000), device="cuda:0"), n_mels, frames=F)
    assert tuple(got.shape) == (3, n_mels, 2 * F)
    g = got.cpu().numpy()
    for b in range(3):
        err = np.abs(g[b] - _ctx_mel(wave[b], F, n_mels)).max()
        print(f"logmel F={F} n_mels={n_mels} v1={v1} clip {b}: max abs err {err:.3e}")
        assert err <= 2e-4, (F, n_mels, v1, b, err)
    if full is not None:
        assert torch.equal(got, full)
    assert torch.isfinite(z).all() and (z == z.flatten()[0]).all()


# ------------------------------------------------------------------------------------------------
# 2. whisper-tiny encoder: time-means of every layer, hidden-state shapes, layer 0 (the conv boundary at 2F)
@pytest.mark.parametrize("F", [1, 16, 37, 150, 160, 161, 200])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_tiny_encoder_context(dtype, F):
    tol, cos_min = BARS[dtype]
    m = _model("tiny", dtype)
    nl = m.spec.layers
    wave = _batch(_lens(F), seed=7)
    ref = _ref_states("tiny", wave, F, "lens3")
    w = torch.from_numpy(wave).cuda()
    idx = list(range(nl + 1))
    emb = m.embed(w, idx, frames=F).cpu().numpy()
    assert emb.shape == (3, nl + 1, m.spec.hidden)
    hs = m.hidden_states(w, frames=F)
    assert len(hs) == nl + 1 and all(tuple(h.shape) == (3, F, m.spec.hidden) for h in hs)
    h0 = hs[0].cpu().numpy()
    for b in range(3):
        means = ref[b].mean(axis=1)
        rel, cos = _rel(emb[b], means), _cos(emb[b], means)
        r0 = np.linalg.norm(h0[b] - ref[b][0]) / np.linalg.norm(ref[b][0])
        print(f"{dtype} F={F} clip {b}: time-mean rel-L2 max {rel.max():.3e} cos min {cos.min():.7f}; layer 0 rel-L2 {r0:.3e}")
        assert rel.max() <= tol and cos.min() >= cos_min, (dtype, F, b, rel, cos)
        assert r0 <= tol, (dtype, F, b, r0)
    # the pooled output is the time-mean of the states the same call materialises
    pooled = torch.stack([h.mean(dim=1) for h in hs], dim=1).cpu().numpy()
    assert _rel(emb, pooled).max() <= (1e-5 if dtype == "fp32" else tol)


# ------------------------------------------------------------------------------------------------
# 3. whisper-small: the split-fp16 and the MX-fp8 paths (257 straddles the fp8 attention's 256-query block;
#    37 < 64 takes the fp8 path's bf16 attention)
@pytest.mark.parametrize("F", [37, 150, 256, 257])
@pytest.mark.parametrize("dtype", ["fp16x3", "fp8"])
def test_small_encoder_context(dtype, F):
    tol, cos_min = BARS[dtype]
    m = _model("small", dtype)
    wave = _batch([48000, F * 320 + 777], seed=23)
    ref = _ref_states("small", wave, F, "lens2")
    idx = m.spec.default_layer_indices() + [0]
    emb = m.embed(torch.from_numpy(wave).cuda(), idx, frames=F).cpu().numpy()
    for b in range(2):
        means = ref[b].mean(axis=1)[idx]
        rel, cos = _rel(emb[b], means), _cos(emb[b], means)
        print(f"{dtype} whisper-small F={F} clip {b}: rel-L2 max {rel.max():.3e} cos min {cos.min():.7f}")
        assert rel.max() <= tol and cos.min() >= cos_min, (dtype, F, b, rel, cos)


@pytest.mark.parametrize("B,F", [(1, 1), (1, 7), (2, 3), (3, 2), (1, 8), (2, 5)])
def test_small_fp8_fewer_rows_than_a_scale_tile(B, F):
    """MX-fp8 with a handful of GEMM rows (M = B F from 1 to 10, on both sides of 8): the A-layout scales of the
    LayerNorm and fc1 outputs are padded to 256-row tiles, 8 K bytes however few rows there are, which is more
    than the M K bytes that follow the e4m3 data in a region sized for bf16 when M < 8 (whisper_plan sizes those
    regions by the padded layout).  Parity at the fp8 bar, each clip bit-equal to the clip alone, and the bytes
    after the workspace untouched."""
    from ssr_amd import _lib
    tol, cos_min = BARS["fp8"]
    m = _model("small", "fp8")
    wave = _batch([48000, F * 320 + 777, 16000][:B], seed=23)
    ref = _ref_states("small", wave, F, f"rows{B}")
    idx = m.spec.default_layer_indices() + [0]
    w = torch.from_numpy(wave).cuda()
    n = m.workspace_bytes(B, w.shape[1], frames=F)
    assert n == _lib.lib().sse_workspace_bytes_ctx(m._h, B, w.shape[1], F)
    guard = 1 << 20
    buf = torch.full((n + guard,), 0x5A, dtype=torch.uint8, device="cuda:0")
    got = m.embed(w, idx, frames=F, workspace=buf[:n])
    torch.cuda.synchronize()
    assert (buf[n:] == 0x5A).all()
    emb = got.cpu().numpy()
    assert np.isfinite(emb).all()
    for b in range(B):
        means = ref[b].mean(axis=1)[idx]
        rel, cos = _rel(emb[b], means), _cos(emb[b], means)
        print(f"fp8 whisper-small B={B} F={F} clip {b}: rel-L2 max {rel.max():.3e} cos min {cos.min():.7f}")
        assert rel.max() <= tol and cos.min() >= cos_min, (B, F, b, rel, cos)
        assert torch.equal(got[b:b + 1], m.embed(w[b:b + 1], idx, frames=F)), (B, F, b)
    assert torch.equal(got, m.embed(w, idx, frames=F))   # the model's own workspace, a second run: no race


@pytest.mark.parametrize("F", [37, 150])
def test_small_bf16_context(F):
    """whisper-small bf16, the path the frames=150 throughput figures are measured on: folded pre-LN (QKV / fc1
    from the p1 / p2 partials, D = 768), 12 heads on the short-T attention."""
    tol, cos_min = BARS["bf16"]
    m = _model("small", "bf16")
    wave = _batch([48000, F * 320 + 777], seed=23)
    ref = _ref_states("small", wave, F, "lens2")
    idx = m.spec.default_layer_indices() + [6, 1, 0]
    emb = m.embed(torch.from_numpy(wave).cuda(), idx, frames=F).cpu().numpy()
    for b in range(2):
        means = ref[b].mean(axis=1)[idx]
        rel, cos = _rel(emb[b], means), _cos(emb[b], means)
        print(f"bf16 whisper-small F={F} clip {b}: rel-L2 max {rel.max():.3e} cos min {cos.min():.7f}")
        assert rel.max() <= tol and cos.min() >= cos_min, (F, b, rel, cos)


# ------------------------------------------------------------------------------------------------
# 4. one-token decoder over the F encoder frames
@pytest.mark.parametrize("F", [37, 150])
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_decoder_context(dtype, F):
    tol, _ = BARS[dtype]
    m = _model("tiny_dec", dtype)
    o = _sd("tiny_dec")[1]
    nd = m.spec.decoder_layers
    c = _batch([48000], seed=41)[0]
    enc_ref = np.stack(o.hidden_states(_ctx_mel(c, F)))
    dec_ref = np.stack(o.decoder_hidden_states(enc_ref[-1]))
    w = torch.from_numpy(np.stack([c, c])).cuda()
    enc_idx, dec_idx = [m.spec.layers, 0], list(range(nd + 1))
    e, d = m.whisper_embed(w, enc_idx, dec_idx, frames=F)
    assert torch.equal(e[0], e[1]) and torch.equal(d[0], d[1])
    re = _rel(e[0].cpu().numpy(), enc_ref.mean(axis=1)[enc_idx]).max()
    rd = _rel(d[0].cpu().numpy(), dec_ref).max()
    print(f"{dtype} F={F}: encoder rel-L2 {re:.3e}, decoder rel-L2 {rd:.3e}")
    assert re <= tol and rd <= tol
    # the decoder-only call takes F from the encoder state's shape
    hs = m.decoder_hidden_states(torch.from_numpy(enc_ref[-1][None]).cuda())
    assert len(hs) == nd + 1 and tuple(hs[0].shape) == (1, 1, m.spec.hidden)
    assert _rel(np.stack([h[0, 0].cpu().numpy() for h in hs]), dec_ref).max() <= tol


# ------------------------------------------------------------------------------------------------
# 5. invariants, all bit-exact
@pytest.mark.parametrize("name,dtype", [("tiny_dec", "fp32"), ("tiny_dec", "bf16"), ("small", "bf16"),
                                        ("small", "fp16x3"), ("small", "fp8")])
def test_full_context_is_the_call_without_one(name, dtype):
    m = _model(name, dtype)
    w = torch.from_numpy(_batch([48000, 30000], seed=3)).cuda()
    idx = [m.spec.layers, 1, 0]
    base = m.embed(w, idx)
    assert torch.equal(base, m.embed(w, idx, frames=1500))
    lens = [48000, 30000]
    assert torch.equal(m.embed(w, idx, lengths=lens), m.embed(w, idx, lengths=lens, frames=1500))
    assert torch.equal(m.embed(w, idx, pool="mean_std", valid_only=True),
                       m.embed(w, idx, pool="mean_std", valid_only=True, frames=1500))
    dec = [0, m.spec.decoder_layers] if m.spec.decoder_layers else []
    e0, d0 = m.whisper_embed(w, idx, dec)
    e1, d1 = m.whisper_embed(w, idx, dec, frames=1500)
    assert torch.equal(e0, e1) and torch.equal(d0, d1) and torch.equal(e0, base)
    a = m.hidden_states(w[:1])
    b = m.hidden_states(w[:1], frames=1500)
    assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_clip_alone_equals_clip_in_batch(dtype):
    m = _model("tiny", dtype)
    idx = list(range(m.spec.layers + 1))
    for F in (37, 150, 200):
        w = torch.from_numpy(_batch(_lens(F), seed=7)).cuda()
        full = m.embed(w, idx, frames=F)
        for b in range(3):
            assert torch.equal(full[b:b + 1], m.embed(w[b:b + 1], idx, frames=F)), (dtype, F, b)


def test_frames_clip_is_the_explicit_integer():
    from ssr_amd.model import logmel
    m = _model("tiny", "bf16")
    idx = [m.spec.layers, 0]
    w = torch.from_numpy(_batch([16000, 48000, 20000], seed=5)).cuda()
    assert m.spec.context_frames(48000) == 150
    assert torch.equal(m.embed(w, idx, frames="clip"), m.embed(w, idx, frames=150))
    assert m.hidden_states(w, frames="clip")[0].shape[1] == 150
    assert torch.equal(logmel(w, frames="clip"), logmel(w, frames=150))
    # with lengths: the context of the longest clip (63 frames), not of the row width
    lens = [16000, 20000, 7000]
    assert m.spec.context_frames(20000) == 63
    assert torch.equal(m.embed(w, idx, lengths=lens, frames="clip"), m.embed(w, idx, lengths=lens, frames=63))
    clips = [w[i, :n] for i, n in enumerate(lens)]
    assert torch.equal(m.embed_clips(clips, idx, frames="clip"), m.embed(w[:, :20000], idx, lengths=lens, frames=63))
    # lengths cut a clip exactly as zero padding does
    w2 = w.clone()
    w2[0, 16000:] = 0
    w2[2, 7000:] = 0
    w2[1, 20000:] = 0
    assert torch.equal(m.embed(w, idx, lengths=lens, frames=63), m.embed(w2, idx, frames=63))


# ------------------------------------------------------------------------------------------------
# 6. composition with the pooling arguments
def test_valid_only_and_windows_with_context():
    m = _model("tiny", "fp32")
    nl = m.spec.layers
    idx = [nl, nl // 2, 0]
    F = 150
    wave = _batch(_lens(F), seed=7)
    ref = _ref_states("tiny", wave, F, "lens3")
    w = torch.from_numpy(wave).cuda()
    lens = _lens(F)
    got = m.embed(w, idx, lengths=lens, valid_only=True, frames=F).cpu().numpy()
    valid = [min(F, -(-n // 320)) for n in lens]
    assert valid == [50, 150, 150]
    for b in range(3):
        rel = _rel(got[b], ref[b][idx, :valid[b]].mean(axis=1)).max()
        print(f"valid_only F={F} clip {b} ({valid[b]} frames): rel-L2 {rel:.3e}")
        assert rel <= 1e-4
    # windows: pool_segments(frames=F) slots, each the fp64 statistics of the hidden states of the same call
    hs = [h.double().cpu() for h in m.hidden_states(w, frames=F)]
    for kw, win, hop in ((dict(), 0, 0), (dict(window=50, hop=25), 50, 25), (dict(window=64, hop=64), 64, 64)):
        S = m.pool_segments(w.shape[1], kw.get("window"), kw.get("hop"), frames=F)
        assert S == _segments(F, win, hop)
        out = m.embed(w, idx, pool="mean_std", frames=F, **kw)
        assert tuple(out.shape) == ((3, 3, S, 2 * m.spec.hidden) if kw else (3, 3, 2 * m.spec.hidden))
        out = out.cpu().reshape(3, 3, S, -1)
        for j, layer in enumerate(idx):
            r, counts = _ref_batch([hs[layer][b] for b in range(3)], None, win, hop, S)
            _check(out[:, j], r, counts, 3, 1, ("ctx", kw, layer))
    assert m.pool_segments(16000, 50, 25, valid_only=True, frames=F) == _segments(50, 50, 25)
    assert m.pool_segments(480000, 50, 25, frames=F) == _segments(F, 50, 25)


# ------------------------------------------------------------------------------------------------
# 7. workspace and errors through the C-ABI
def test_workspace_scales_with_the_context():
    from ssr_amd import _lib
    L = _lib.lib()
    for name, dtype in (("tiny_dec", "fp32"), ("small", "bf16"), ("small", "fp8"), ("small", "fp16x3")):
        m = _model(name, dtype)
        full = L.sse_workspace_bytes(m._h, 8, 48000)
        sizes = [L.sse_workspace_bytes_ctx(m._h, 8, 48000, F) for F in range(1, 1501)]
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
        assert sizes[-1] == full
        assert sizes[149] < full / 5, (name, dtype, sizes[149], full)
        assert m.workspace_bytes(8, 48000, frames=150) == sizes[149] and m.workspace_bytes(8, 48000) == full
        assert L.sse_output_frames_ctx(m._h, 48000, 150) == 150 and L.sse_output_frames(m._h, 48000) == 1500
        for n, f in ((0, 1), (1, 1), (320, 1), (321, 2), (48000, 150), (480000, 1500), (500000, 1500)):
            assert L.sse_whisper_context_frames(m._h, n) == f == m.spec.context_frames(n)


def test_c_abi_context_errors(wavlm_sd):
    from ssr_amd import _lib, config as C
    from ssr_amd.model import SSEModel
    L = _lib.lib()
    m = _model("tiny_dec", "bf16")
    H = m.spec.hidden
    w = torch.from_numpy(_batch([48000, 30000], seed=3)).cuda()
    ids = torch.tensor([4, 0], dtype=torch.int32)
    mark = 1234.5
    out = torch.full((2, 2, 1500, H), mark, device="cuda")
    ws = m.workspace(2, 48000)
    s = m._stream()
    desc = _lib.sse_pool_desc(1, 1, 0, 0, 0)

    def calls(h, F, ws_bytes):
        return {"embed_pooled": L.sse_embed_pooled_ctx(h, w.data_ptr(), None, 2, 48000, F, ids.data_ptr(), 2,
                                                       ctypes.byref(desc), out.data_ptr(), ws.data_ptr(), ws_bytes, s),
                "embed": L.sse_embed_pooled_ctx(h, w.data_ptr(), None, 2, 48000, F, ids.data_ptr(), 2, None,
                                                out.data_ptr(), ws.data_ptr(), ws_bytes, s),
                "hidden_states": L.sse_hidden_states_ctx(h, w.data_ptr(), 2, 48000, F, out.data_ptr(), ws.data_ptr(),
                                                         ws_bytes, s),
                "from_mel": L.sse_whisper_hidden_states_from_mel_ctx(h, w.data_ptr(), 2, F, out.data_ptr(),
                                                                     ws.data_ptr(), ws_bytes, s),
                "whisper_embed": L.sse_whisper_embed_ctx(h, w.data_ptr(), 2, 48000, F, ids.data_ptr(), 2, out.data_ptr(),
                                                         ids.data_ptr(), 2, out.data_ptr(), ws.data_ptr(), ws_bytes, s),
                "decoder": L.sse_whisper_decoder_hidden_states_ctx(h, w.data_ptr(), 2, F, out.data_ptr(), ws.data_ptr(),
                                                                   ws_bytes, s)}

    for F in (0, -1, 1501, 1 << 30):
        for what, rc in calls(m._h, F, ws.numel()).items():
            assert rc == _lib.SSE_ERR_INVALID, (what, F, rc)
        assert L.sse_workspace_bytes_ctx(m._h, 2, 48000, F) == 0
        assert L.sse_output_frames_ctx(m._h, 48000, F) == _lib.SSE_ERR_INVALID
        assert L.sse_pool_out_floats_ctx(m._h, 2, 48000, F, 2, ctypes.byref(desc)) == 0
        assert L.sse_logmel_workspace_bytes_ctx(2, 80, F) == 0
        assert L.sse_logmel_ctx(w.data_ptr(), 2, 48000, 80, F, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                s) == _lib.SSE_ERR_INVALID
    wav = SSEModel(C.WAVLM_BASE, wavlm_sd, device="cuda:0", dtype="bf16")
    for what, rc in calls(wav._h, 150, ws.numel()).items():
        assert rc == _lib.SSE_ERR_INVALID, (what, "wavlm", rc)
    assert L.sse_workspace_bytes_ctx(wav._h, 2, 48000, 150) == 0
    assert L.sse_whisper_context_frames(wav._h, 48000) == _lib.SSE_ERR_INVALID
    # a workspace sized for a smaller context
    small = L.sse_workspace_bytes_ctx(m._h, 2, 48000, 37)
    for what, rc in calls(m._h, 150, small).items():
        assert rc == _lib.SSE_ERR_WORKSPACE, (what, rc)
    torch.cuda.synchronize()
    assert (out == mark).all()
    # ... and the same calls go through with the right one
    assert L.sse_pool_out_floats_ctx(m._h, 2, 48000, 150, 2, ctypes.byref(desc)) == 2 * 2 * H
    assert L.sse_embed_pooled_ctx(m._h, w.data_ptr(), None, 2, 48000, 150, ids.data_ptr(), 2, None, out.data_ptr(),
                                  ws.data_ptr(), L.sse_workspace_bytes_ctx(m._h, 2, 48000, 150), s) == 0
    torch.cuda.synchronize()
    flat = out.flatten()
    assert torch.isfinite(flat[:2 * 2 * H]).all() and (flat[:2 * 2 * H] != mark).any() and (flat[2 * 2 * H:] == mark).all()
    assert torch.equal(flat[:2 * 2 * H].view(2, 2, H), m.embed(w, [4, 0], frames=150))


# ------------------------------------------------------------------------------------------------
# 8. the reference-shaped surface passes the context through
def test_glue_passes_frames_through():
    from ssr_amd import corpus, extract, hf
    m = _model("tiny_dec", "fp32")
    model = hf.WhisperModel(m)
    proc = hf.WhisperProcessor(device="cuda:0")
    c = _batch([48000], seed=41)[0]
    w = torch.from_numpy(c).cuda()[None]
    enc_idx, dec_idx = [4, 3], [4, 0]
    e, d = m.whisper_embed(w, enc_idx, dec_idx, frames=150)
    names = [f"encoder_layer_{i}" for i in enc_idx] + [f"decoder_layer_{i}" for i in dec_idx]
    for frames in (150, "clip"):
        out = extract.extract_embeddings_from_audio_whisper(c, model, proc, "cuda:0", names, frames=frames)
        for j, i in enumerate(enc_idx):
            assert np.array_equal(out[f"encoder_layer_{i}"], e[0, j].cpu().numpy())
        for j, i in enumerate(dec_idx):
            assert np.array_equal(out[f"decoder_layer_{i}"], d[0, j].cpu().numpy())
    with pytest.raises(ValueError):
        extract.extract_embeddings_from_audio_whisper(c, model, proc, "cuda:0", names, frames=0)
    assert torch.equal(model.embed(w, enc_idx, frames=150), e)
    # the duck-typed encoder on input_features of width 2F, the decoder on its [B, F, H] output
    feats = proc(c, sampling_rate=16000, frames=150).input_features
    assert tuple(feats.shape) == (1, 80, 300)
    eo = model.encoder(feats, output_hidden_states=True)
    hs = m.hidden_states(w, frames=150)
    assert all(torch.equal(a, b) for a, b in zip(eo.hidden_states, hs))
    do = model.decoder(input_ids=torch.zeros((1, 1), dtype=torch.long), encoder_hidden_states=eo.last_hidden_state,
                       output_hidden_states=True)
    assert _rel(do.hidden_states[4][0, 0].cpu().numpy(), d[0, 0].cpu().numpy()) <= 1e-5
    fn = corpus.sse_embed_fn(m, enc_idx, frames=150)
    assert torch.equal(fn(w), e)
