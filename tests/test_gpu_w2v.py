"""wav2vec 2.0 / HuBERT on the GPU: the WavLM encoder without the gated relative-position bias
(``WavLMSpec(num_buckets=0)``: no gate columns in the QKV GEMM, the attention kernels' bias-free instantiations).

Two independent checks:
* the reference's own glue on transformers' Wav2Vec2Model / HubertModel (tests/golden/wav2vec2_base.npz,
  hubert_large4.npz; tests/test_w2v_cpu.py pins the fixtures to the numpy oracle) at the project's bars
  (tests/test_gpu_wavlm.py, tests/test_gpu_wavlm_fp8.py);
* the OLD route to the same function -- a WavLM-kind spec with a zero ``rel_attn_embed`` and random gate tensors,
  which runs the gated-bias kernels this repository already tests -- at 1e-5 in fp32 (same arithmetic, another
  route) and in the folded-LayerNorm tests' form for the 16-bit paths.

Bars: fp32 / fp16x3 rel-L2 <= 1e-4; fp16 <= 5e-3; bf16 <= 3e-2 and cosine >= 0.999; fp8 <= 0.08 and cosine >= 0.995
(large shape only); pooling: 1e-5 of max|ref| per output vector, max bit-equal (tests/test_gpu_pooling.py)."""
import dataclasses

import numpy as np
import pytest
import torch

import w2v_fixtures as wf
from test_gpu_pooling import _check_layers, _folded
from test_wavio import write_wav

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-4
FP16_TOL = 5e-3
BF16_TOL, BF16_COS = 3e-2, 0.999
FP8_TOL, FP8_COS = 0.08, 0.995
ROUTE_FP32_TOL = 1e-5
ROUTE_16_TOL = 2e-2
TOL = {"fp32": FP32_TOL, "fp16x3": FP32_TOL, "fp16": FP16_TOL, "bf16": BF16_TOL, "fp8": FP8_TOL}

_MODELS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    """The cached models live for this module only: free them (and torch's cached blocks) afterwards, so the
    modules that run next see the device as they would without this file."""
    yield
    import gc
    for m in _MODELS.values():
        m.close()
    _MODELS.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _rel(a, b):
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


def _cos(a, b):
    return (a * b).sum(-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def _model(name, dtype, route="new"):
    """wav2vec2_base (12 layers, post-LN) or hubert_large4 (stable-LN, conv biases, do_normalize) on the new
    (num_buckets=0) or the old (zero table) route; built once per module."""
    from ssr_amd.model import SSEModel
    key = (name, dtype, route)
    if key not in _MODELS:
        spec = {"wav2vec2_base": wf.W2V_SPEC, "hubert_large4": wf.HUB_SPEC}[name]
        sd = wf.weights(name)
        if route == "old":
            spec, sd = wf.old_route(spec, sd)
        _MODELS[key] = SSEModel(spec, sd, device="cuda:0", dtype=dtype, do_normalize=name == "hubert_large4")
    return _MODELS[key]


def _at_bar(got, ref, dtype, what):
    rel, cos = _rel(got, ref).max(), _cos(got, ref).min()
    print(what, dtype, "rel-L2", rel, "cos", cos)
    assert np.isfinite(got).all(), what
    assert rel <= TOL[dtype], (what, dtype, rel)
    if dtype == "bf16":
        assert cos >= BF16_COS, (what, cos)
    if dtype == "fp8":
        assert cos >= FP8_COS, (what, cos)


# ---- the reference's fixtures ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "fp16x3", "fp16", "bf16"])
def test_wav2vec2_base_matches_reference(dtype):
    g = wf.golden("wav2vec2_base")
    m = _model("wav2vec2_base", dtype)
    assert m.spec.num_buckets == 0 and m.output_frames(48000) == 149
    idx = [int(i) for i in g["layer_indices"]]
    got = m.embed(torch.from_numpy(wf.clips("wav2vec2_base", "emb")).cuda(), idx).cpu().numpy()
    assert got.shape == (4, 13, 768)
    _at_bar(got, g["emb"], dtype, "wav2vec2-base pooled")
    if dtype in ("fp32", "fp16x3"):
        hs = m.hidden_states(torch.from_numpy(wf.clips("wav2vec2_base", "hs_short")).cuda())
        assert len(hs) == 13 and tuple(hs[0].shape) == (1, 49, 768)
        for i in (0, 1, 12):
            ref = g[f"hs{i}_short"]
            rel = np.linalg.norm(hs[i][0].cpu().numpy() - ref) / np.linalg.norm(ref)
            print("hidden_states", i, dtype, rel)
            assert rel <= FP32_TOL, (i, rel)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_wav2vec2_base_long_clip_matches_reference(dtype):
    """56,000 samples = 174 frames, past the 160-frame split: the long-T bias-free kernels
    (bf16: attention_flash2_kernel<false>; fp32: attention_kernel<float, false>)."""
    g = wf.golden("wav2vec2_base")
    m = _model("wav2vec2_base", dtype)
    assert m.output_frames(56000) == 174
    got = m.embed(torch.from_numpy(wf.clips("wav2vec2_base", "emb_long")).cuda(), list(range(13))).cpu().numpy()
    _at_bar(got[0], g["emb_long"], dtype, "wav2vec2-base 174 frames")


@pytest.mark.parametrize("dtype", ["fp32", "fp16x3", "fp16", "bf16", "fp8"])
def test_hubert_large_matches_reference(dtype):
    """The large shape cut to 4 layers: conv biases + layer-norm frontend (hidden_states[0]), stable-LN encoder,
    do_normalize; fp8 (stable-LN only) runs the MX-fp8 QKV GEMM over all 3072 = q | k | v columns."""
    g = wf.golden("hubert_large4")
    m = _model("hubert_large4", dtype)
    idx = [int(i) for i in g["layer_indices"]]
    got = m.embed(torch.from_numpy(wf.clips("hubert_large4", "emb")).cuda(), idx).cpu().numpy()
    assert got.shape == (3, 5, 1024)
    _at_bar(got, g["emb"], dtype, "hubert-large4 pooled")
    if dtype in ("fp32", "fp16x3"):
        h0 = m.hidden_states(torch.from_numpy(wf.clips("hubert_large4", "hs_short")).cuda())[0][0].cpu().numpy()
        ref = g["hs0_short"]
        rel = np.linalg.norm(h0 - ref) / np.linalg.norm(ref)
        print("hubert hidden_states[0]", dtype, rel)
        assert h0.shape == (49, 1024) and rel <= FP32_TOL


# ---- two routes to the same function --------------------------------------------------------------------------
ROUTE_SHAPES = [(5, 16000), (3, 48000), (2, 56000)]     # B = 5 at 49 frames, 3 at 149, 2 at 174


def _route_clips(name, B, L):
    from ssr_amd import synth
    if name == "wav2vec2_base" and (B, L) == (3, 48000):
        return wf.clips(name, "emb")[:3]                 # the fixture's own clips: errors against the fixture too
    return synth.synth_clips(B, L, seed=4000 + B)


@pytest.mark.parametrize("name", ["wav2vec2_base", "hubert_large4"])
def test_two_routes_fp32(name):
    """Same arithmetic, another route (gate columns computed and multiplied by a zero table): <= 1e-5."""
    new, old = _model(name, "fp32"), _model(name, "fp32", "old")
    idx = list(range(new.spec.layers + 1))
    for B, L in ROUTE_SHAPES:
        w = torch.from_numpy(_route_clips(name, B, L)).cuda()
        a, b = new.embed(w, idx).cpu().numpy(), old.embed(w, idx).cpu().numpy()
        rel = _rel(a, b).max()
        print(name, "fp32 routes", (B, L), rel)
        assert np.isfinite(a).all() and rel <= ROUTE_FP32_TOL, (B, L, rel)
        ha, hb = new.hidden_states(w[:1]), old.hidden_states(w[:1])
        for x, y in zip(ha, hb):
            assert _rel(x.cpu().numpy().reshape(-1), y.cpu().numpy().reshape(-1)) <= ROUTE_FP32_TOL


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("name", ["wav2vec2_base", "hubert_large4"])
def test_two_routes_16bit(name, dtype):
    """Two 16-bit paths with different GEMM widths (and, post-LN, different folded weights): compared by
    tolerance (<= 2e-2) and by their distance to the truth -- the new route no farther than 1.25 x the old
    route's + 1e-3 (the folded-LayerNorm tests' form).  The truth is the fp32 model of the new route (itself
    within 1e-4 of the fixture), and the fixture itself on the fixture's clips."""
    new, old, m32 = _model(name, dtype), _model(name, dtype, "old"), _model(name, "fp32")
    idx = list(range(new.spec.layers + 1))
    g = wf.golden(name)
    for B, L in ROUTE_SHAPES:
        w = torch.from_numpy(_route_clips(name, B, L)).cuda()
        a, b, r = (m.embed(w, idx).cpu().numpy() for m in (new, old, m32))
        e_a, e_b = _rel(a, r).max(), _rel(b, r).max()
        print(name, dtype, (B, L), "routes", _rel(a, b).max(), "| vs fp32: new", e_a, "old", e_b)
        assert np.isfinite(a).all() and _rel(a, b).max() <= ROUTE_16_TOL
        assert e_a <= 1.25 * e_b + 1e-3 and e_a <= TOL[dtype]
        if name == "wav2vec2_base" and (B, L) == (3, 48000):
            f_a, f_b = _rel(a, g["emb"][:3]).max(), _rel(b, g["emb"][:3]).max()
            print(name, dtype, "vs fixture: new", f_a, "old", f_b)
            assert f_a <= 1.25 * f_b + 1e-3


# ---- ragged batches, the half-batch split ---------------------------------------------------------------------
def _ragged(lens, seed):
    from ssr_amd import synth
    rng = np.random.default_rng(seed)
    wave = rng.standard_normal((len(lens), max(lens))).astype(np.float32) * 3.0     # garbage past each clip's end
    clips = [synth.synth_clips(1, n, seed=seed + i)[0] for i, n in enumerate(lens)]
    for i, c in enumerate(clips):
        wave[i, :len(c)] = c
    return torch.from_numpy(wave).cuda(), clips


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("name", ["wav2vec2_base", "hubert_large4"])
def test_ragged_equals_solo(name, dtype):
    """49, 149 and 174 frames in one batch, on both sides of the 160-frame split (bf16: the short-T kernel and
    the flash kernel each take their clips): every clip is bit-equal to its solo call."""
    m = _model(name, dtype)
    lens = [16000, 48000, 56000]
    idx = [m.spec.layers, m.spec.layers // 2, 0]
    wave, clips = _ragged(lens, 610)
    got = m.embed(wave, idx, lengths=lens)
    assert torch.isfinite(got).all()
    for i, c in enumerate(clips):
        assert torch.equal(got[i:i + 1], m.embed(torch.from_numpy(c).cuda()[None], idx)), (name, dtype, lens[i])
    ec = m.embed_clips([torch.from_numpy(c) for c in clips], idx)
    assert torch.equal(ec, got)


def test_half_batch_split_equals_solo():
    """B = 128 runs as two half-batches on two streams, each with its own (narrower) workspace plan."""
    from ssr_amd import synth
    m = _model("wav2vec2_base", "bf16")
    w = torch.from_numpy(synth.synth_clips(128, 16000, seed=88)).cuda()
    full = m.embed(w, [12, 6])
    assert torch.isfinite(full).all()
    for i in (0, 63, 64, 127):
        assert torch.equal(full[i:i + 1], m.embed(w[i:i + 1], [12, 6])), i


# ---- pooling --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_pooled_matches_hidden_states(dtype):
    """pool="mean_std_max", whole clip and window=50 / hop=25 (149 frames: 5 segments), against fp64 pooling of
    hidden_states() of the same model (tests/test_gpu_pooling.py's reference and bars)."""
    from ssr_amd.model import pool_states
    m = _model("wav2vec2_base", dtype)
    idx = [12, 6, 0]
    wave = torch.from_numpy(wf.clips("wav2vec2_base", "emb")[:3]).cuda()
    hs_dev = m.hidden_states(wave)
    hs = [h.double().cpu() for h in hs_dev]
    per_clip = [[h[b] for h in hs] for b in range(3)]
    folded = _folded(dtype, 12)
    full = m.embed(wave, idx, pool="mean_std_max")
    assert tuple(full.shape) == (3, 3, 3 * 768)
    _check_layers(full, per_clip, idx, folded, 0, 0, (dtype, "full"))
    wind = m.embed(wave, idx, pool="mean_std_max", window=50, hop=25)
    assert tuple(wind.shape) == (3, 3, 5, 3 * 768) and m.pool_segments(48000, 50, 25) == 5
    _check_layers(wind, per_clip, idx, folded, 50, 25, (dtype, "window"))
    # and against the stand-alone kernel on the materialised states, pool_states(hidden_states()), same bars
    H = 768
    for got, kw in ((full[:, :, None], {}), (wind, dict(window=50, hop=25))):
        for j, layer in enumerate(idx):
            ref = pool_states(hs_dev[layer], None, "mean_std_max", **kw).reshape(3, -1, 3 * H).double()
            g = got[:, j].double()
            for k in range(3):   # mean, std, max
                a, r = g[..., k * H:(k + 1) * H], ref[..., k * H:(k + 1) * H]
                if k == 2 and layer not in folded:
                    assert torch.equal(a, r), (dtype, layer, kw)
                else:
                    assert ((a - r).abs().amax(-1) <= 1e-5 * r.abs().amax(-1)).all(), (dtype, layer, k, kw)
    assert torch.equal(m.embed(wave, idx, pool="mean"), m.embed(wave, idx))
    with pytest.raises(ValueError, match="Whisper"):
        m.embed(wave, idx, frames=100)


# ---- the reference-shaped loop --------------------------------------------------------------------------------
def test_dropin_hubert_reproduces_fixture(tmp_path):
    """extract_wavlm_embeddings (file in, dict out) with hf.Wav2Vec2FeatureExtractor + hf.HubertModel: the fused
    route and the generic model(...).hidden_states route, against hubert_large4.npz at 1e-4."""
    from ssr_amd import hf
    from ssr_amd.extract import extract_wavlm_embeddings
    g = wf.golden("hubert_large4")
    model = hf.HubertModel.from_state_dict(wf.HUB_SPEC, wf.weights("hubert_large4"), device="cuda:0", dtype="fp32")
    fe = hf.Wav2Vec2FeatureExtractor(do_normalize=True, device="cuda:0")
    assert isinstance(model, hf.WaveEncoderModel) and model.config.hidden_size == 1024
    idx = [int(i) for i in g["layer_indices"]]
    clips = wf.clips("hubert_large4", "emb")
    for i in range(2):
        p = str(tmp_path / f"h{i}.wav")
        write_wav(p, clips[i], fmt="float")
        d = extract_wavlm_embeddings(p, model, fe, "cuda:0", idx)
        assert list(d) == [f"layer_{j}" for j in idx]
        for j, k in enumerate(idx):
            assert d[f"layer_{k}"].dtype == np.float32 and d[f"layer_{k}"].shape == (1024,)
            assert _rel(d[f"layer_{k}"], g["emb"][i, j]) <= FP32_TOL, (i, k)
    inputs = fe(clips[0], sampling_rate=16000, return_tensors="pt").to("cuda:0")
    out = model(inputs.input_values, output_hidden_states=True, return_dict=True)
    assert len(out.hidden_states) == 5 and tuple(out.hidden_states[0].shape) == (1, 149, 1024)
    for j, k in enumerate(idx):
        v = torch.mean(out.hidden_states[k], dim=1).cpu().numpy().flatten()
        assert _rel(v, g["emb"][0, j]) <= FP32_TOL
    with pytest.raises(NotImplementedError):
        model(inputs.input_values, attention_mask=torch.ones_like(inputs.input_values))


def test_from_hf_takes_transformers_models():
    """Wav2Vec2Model.from_hf / HubertModel.from_hf on transformers' own objects (2 layers, random init, extra
    masked_spec_embed key): the twin's hidden states equal transformers' own forward of a 1 s clip on the CPU."""
    from transformers import HubertConfig, HubertModel, Wav2Vec2Config, Wav2Vec2Model
    from ssr_amd import hf
    torch.manual_seed(0)
    w = torch.from_numpy(wf.clips("wav2vec2_base", "hs_short")).cuda()
    big = dict(hidden_size=1024, num_hidden_layers=2, num_attention_heads=16, intermediate_size=4096,
               feat_extract_norm="layer", do_stable_layer_norm=True, conv_bias=True)
    for twin, ref in ((hf.Wav2Vec2Model, Wav2Vec2Model(Wav2Vec2Config(num_hidden_layers=2))),
                      (hf.HubertModel, HubertModel(HubertConfig(**big)))):
        t = twin.from_hf(ref.eval(), device="cuda:0", dtype="fp32")
        assert t.sse.spec.num_buckets == 0 and t.sse.spec.layers == 2
        got = t(w, output_hidden_states=True).hidden_states
        with torch.no_grad():
            want = ref(w.cpu(), output_hidden_states=True).hidden_states
        for a, b in zip(got, want):
            assert _rel(a.cpu().numpy().reshape(-1), b.numpy().reshape(-1)) <= FP32_TOL


# ---- error codes ----------------------------------------------------------------------------------------------
def test_error_codes():
    from ssr_amd import _lib
    from ssr_amd.model import SSEModel
    with pytest.raises(_lib.SSEError) as e:
        SSEModel(wf.W2V_SPEC, wf.weights("wav2vec2_base"), device="cuda:0", dtype="fp8")     # post-LN: refused
    assert e.value.rc == _lib.SSE_ERR_UNSUPPORTED
    xl = dataclasses.replace(wf.HUB_SPEC, hidden=1280, ffn=5120, name="head-width-80")
    with pytest.raises(ValueError, match="head width of 64"):
        SSEModel(xl, {}, device="cuda:0")
