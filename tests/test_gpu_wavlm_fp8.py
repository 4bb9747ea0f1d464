"""WavLM-large with dtype="fp8": the stable-LN encoder's QKV / fc1 / fc2 GEMMs on the MX-fp8 matrix core, bf16
activations, attention, out-projection and residual stream (SSE_DTYPE_FP8 for SSE_KIND_WAVLM).

Bars (written here, stated in DESIGN.md §4):
* embeddings against the reference's fixture, the fp32 model of the same weights and the bf16 model: the project's
  fp8 bar, rel-L2 <= 0.08 and cosine >= 0.995 (tests/test_gpu_mx.py); the format-forced error of the reference
  arithmetic alone is 0.0589 / 0.99827 on the fixture's inputs (tools/wavlm_mx_emulate.py);
* batch, ragged and two-stream invariance: bit-equal (MX scales are per row and per 32 columns, and a row's
  accumulation order does not depend on its position in a tile);
* pooling against hidden_states(): tests/test_gpu_pooling.py's bar, 1e-5 of max|ref| per output vector;
* the MX GEMM at WavLM-large's shapes: <= 1e-4 of max|C| against the fp64 product of the dequantised operands, bf16
  output equal to the rounded fp32 one (test_gemm_mx_matches_dequantised_product's criterion), guard rows untouched.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from oracle import mx

pytestmark = pytest.mark.gpu

FP8_TOL, FP8_COS = 0.08, 0.995
IDX = [24, 23, 22, 12]


def _rel(a, b):
    return np.linalg.norm(a - b, axis=-1) / np.linalg.norm(b, axis=-1)


def _cos(a, b):
    return np.sum(a * b, axis=-1) / (np.linalg.norm(a, axis=-1) * np.linalg.norm(b, axis=-1))


def _at_bar(got, ref, what):
    got, ref = got.cpu().numpy() if isinstance(got, torch.Tensor) else got, \
        ref.cpu().numpy() if isinstance(ref, torch.Tensor) else ref
    rel, cos = _rel(got, ref).max(), _cos(got, ref).min()
    print(what, "rel-L2", rel, "cos", cos)
    assert np.isfinite(got).all(), what
    assert rel <= FP8_TOL and cos >= FP8_COS, (what, rel, cos)


@pytest.fixture(scope="module")
def sd():
    from ssr_amd import config as C, synth
    return synth.synth_wavlm_state_dict(C.WAVLM_LARGE, seed=9)


@pytest.fixture(scope="module")
def fixture_clips():
    from ssr_amd import synth
    return torch.from_numpy(synth.synth_clips(3, 48000, seed=77)).cuda()


def _model(sd, dtype):
    from ssr_amd import config as C
    from ssr_amd.model import SSEModel
    return SSEModel(C.WAVLM_LARGE, sd, device="cuda:0", dtype=dtype, do_normalize=True)


@pytest.fixture(scope="module")
def bf16_before(sd, fixture_clips):
    """A bf16 model built and run before any fp8 WavLM model of this module: (model, its fixture embeddings)."""
    m = _model(sd, "bf16")
    return m, m.embed(fixture_clips, IDX).clone()


@pytest.fixture(scope="module")
def m8(sd, bf16_before):
    return _model(sd, "fp8")   # raises on a build without the feature


@pytest.fixture(scope="module")
def m32(sd):
    return _model(sd, "fp32")


def _ragged(lens, seed):
    """Rows of random values with each clip's samples at the front -> (wave [B, max(lens)] on the GPU, clips)."""
    from ssr_amd import synth
    rng = np.random.default_rng(seed)
    wave = rng.standard_normal((len(lens), max(lens))).astype(np.float32) * 3.0
    clips = [synth.synth_clips(1, n, seed=seed + i)[0] for i, n in enumerate(lens)]
    for i, c in enumerate(clips):
        wave[i, :len(c)] = c
    return torch.from_numpy(wave).cuda(), [torch.from_numpy(c).cuda()[None] for c in clips]


def test_fixture_parity(m8, fixture_clips):
    """The reference's own embeddings of these clips (tests/golden/wavlm_large.npz); measured value in DESIGN.md §4."""
    g = np.load(os.path.join(GOLDEN, "wavlm_large.npz"))
    assert [int(i) for i in g["layer_indices"]] == IDX
    _at_bar(m8.embed(fixture_clips, IDX), g["emb"], "fp8 wavlm-large vs reference fixture")


def test_distance_to_bf16(m8, bf16_before, fixture_clips):
    """fp8 is a perturbation of the same function: its distance to the bf16 path is within the fixture bar."""
    _at_bar(m8.embed(fixture_clips, IDX), bf16_before[1], "fp8 vs bf16")


@pytest.mark.parametrize("lens", [[400], [400, 12345, 48000], [16000]], ids=["T1", "ragged", "1s"])
def test_smallest_shapes(m8, m32, lens):
    """M = 1 (one 400-sample clip is one frame: the operand regions are sized by their 256-row scale tiles, not by
    M), a ragged batch of 1, 38 and 149 frames, and a 1 s clip: finite, and at the fp8 bar against the fp32 model."""
    wave, _ = _ragged(lens, 500 + len(lens))
    kw = dict(lengths=lens) if len(lens) > 1 else {}
    _at_bar(m8.embed(wave, IDX, **kw), m32.embed(wave, IDX, **kw), f"fp8 vs fp32 {lens}")


def test_batch_and_ragged_invariance(m8):
    from ssr_amd import synth
    w = torch.from_numpy(synth.synth_clips(5, 48000, seed=31)).cuda()
    full = m8.embed(w, IDX)
    for i in range(5):
        assert torch.equal(full[i:i + 1], m8.embed(w[i:i + 1], IDX)), i
    lens = [48000, 400, 12345, 47999, 30000]
    wave, clips = _ragged(lens, 300)
    got = m8.embed(wave, IDX, lengths=lens)
    assert torch.isfinite(got).all()
    for i, c in enumerate(clips):
        assert torch.equal(got[i:i + 1], m8.embed(c, IDX)), (i, lens[i])


@pytest.mark.parametrize("samples", [16000, 48000])
def test_two_stream_split_equals_one_stream(m8, samples):
    """B >= 128 runs as two half-batches, each with its own operand and scale regions in its workspace slice:
    bit-equal to the one-stream call, full-length and ragged.

    48000 samples (test_gpu_wavlm.py's split shape, 9834 rows per half) is bit-equal.  16000 samples (3234 rows per
    half) is NOT reliably bit-equal, and not because of the fp8 path: measured on an MI355X, the split call of
    WavLM-large differs from the one-stream call in 0-24 clips of the second half, from hidden state 0 (the conv
    front end, before any encoder layer) on, in 9 of 10 calls, max |diff| 0.26 -- for dtype="bf16" (the
    launches of the parent commit) exactly as for "fp8", also at 200 clips of 8000 samples (2400 rows per half), never
    at >= 4092 rows per half, never for WavLM-base, never without the split; each half alone is bit-equal to its
    rows of the whole batch, stores nothing outside its workspace slice and reads no byte it did not write.  With the
    halves on disjoint CUs (option split_cumask = 1 or 2) 0 of 20 calls differ, with gemm_nonpersist = 1 (no persistent
    8-phase GEMM) 1 of 10, by default 9 of 10.  Two no_split calls of the halves on two torch streams with separately
    allocated workspaces show the same, always in the call issued second: the later call's front end is disturbed by
    the earlier call's encoder-layer kernels when they share CUs at these small grids.  One kernel type at a time on
    the other stream: the persistent 8-phase GEMM in its fc1 form (3234 x 4096 x 1024) disturbs 42-48 of 65 clips in 8
    of 8 trials; attention, out-projection and the LayerNorm -> MX producer never do.  How it reaches the other call's
    LayerNorm front end is not found (DESIGN.md §3 "MX-fp8 for stable-LN WavLM"); the case stays as the feature's
    specification states it."""
    from ssr_amd import _lib, synth
    w = torch.from_numpy(synth.synth_clips(131, samples, seed=17)).cuda()
    for kw in (dict(), dict(lengths=[samples - 97 * i for i in range(131)])):
        a = m8.embed(w, IDX, **kw)
        with _lib.option("no_split", 1):
            b = m8.embed(w, IDX, **kw)
        assert torch.isfinite(a).all() and torch.equal(a, b), kw


def test_pooling_and_hidden_states(m8):
    from ssr_amd import synth
    w = torch.from_numpy(synth.synth_clips(3, 16000, seed=21)).cuda()
    hs = m8.hidden_states(w)
    assert len(hs) == 25 and tuple(hs[0].shape) == (3, 49, 1024)
    got = m8.embed(w, IDX, pool="mean_std").cpu().double()
    assert tuple(got.shape) == (3, 4, 2048)
    for j, layer in enumerate(IDX):
        h = hs[layer].double().cpu()
        for k, ref in enumerate((h.mean(1), h.std(1, correction=1))):
            err = (got[:, j, 1024 * k:1024 * (k + 1)] - ref).abs().amax(-1)
            assert (err <= 1e-5 * ref.abs().amax(-1)).all(), (layer, k, float(err.max()))
    # windows: the first window's mean is the mean of its frames
    wind = m8.embed(w, IDX, pool="mean", window=16, hop=8).cpu().double()
    ref = hs[IDX[1]].double().cpu()[:, :16].mean(1)
    assert ((wind[:, 1, 0] - ref).abs().amax(-1) <= 1e-5 * ref.abs().amax(-1)).all()


class _Guarded:
    """[rows + 8, n] filled with a NaN bit pattern; .out is the first `rows` rows, the rest the canary."""
    PAT = {torch.float32: (torch.int32, 0x7FC0BEEF), torch.bfloat16: (torch.int16, 0x7FB5), torch.uint8: (torch.uint8, 0xA5)}

    def __init__(self, rows, n, dt):
        iv, pat = self.PAT[dt]
        self.rows, self.pat = rows, pat
        self.raw = torch.full((rows + 8, n), pat, dtype=iv, device="cuda")
        self.out = self.raw.view(dt)[:rows]

    def check(self, what):
        torch.cuda.synchronize()
        assert bool((self.raw[self.rows:] == self.pat).all()), f"{what}: store past row M"


def _gemm_ex(M, N, K, a, a_s, b, b_s, zero, **kw):
    from ssr_amd import _lib
    d = _lib.sse_gemm_desc()
    d.dtype, d.M, d.N, d.K, d.ldc, d.act = _lib.SSE_DTYPE_FP8, M, N, K, N, kw.pop("act", 0)
    d.a, d.b, d.a_scale, d.b_scale, d.zero = a.data_ptr(), b.data_ptr(), a_s.data_ptr(), b_s.data_ptr(), zero.data_ptr()
    for k, v in kw.items():
        setattr(d, k, v.data_ptr())
    _lib.check(_lib.lib().sse_gemm_ex(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)),
               "sse_gemm_ex")


@pytest.mark.parametrize("M,N,K", [(1, 3328, 1024), (149, 3328, 1024), (447, 4096, 1024), (447, 1024, 4096)])
def test_gemm_mx_wavlm_large_shapes(M, N, K):
    """The MX GEMM's four outputs at WavLM-large's shapes (N = ldq = 3328 is 13 column tiles; row tiles not full):
    fp32, bf16 (the QKV form), MX-fp8 with GELU (fc1) and the bf16 residual stream in place (fc2)."""
    from ssr_amd.model import mx_scale_bytes
    rng = np.random.default_rng(M + N + K)
    a = rng.standard_normal((M, K)).astype(np.float32)
    b = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)
    qa, sa, ea = mx.quantize(a, 0)
    qb, sb, eb = mx.quantize(b, 1)
    ref = mx.dequantize(qa, ea).astype(np.float64) @ mx.dequantize(qb, eb).astype(np.float64).T
    dev = lambda v: torch.from_numpy(v).cuda()   # noqa: E731
    ops = (dev(qa), dev(sa), dev(qb), dev(sb))
    bias_h = rng.standard_normal(N).astype(np.float32)
    bias, zero = dev(bias_h), torch.zeros(64, device="cuda")
    scale = np.abs(ref).max()
    # fp32 and bf16 (QKV form: bias, no activation)
    f = _Guarded(M, N, torch.float32)
    _gemm_ex(M, N, K, *ops, zero, bias=bias, cf=f.out)
    f.check("fp32 out")
    err = np.abs(f.out.cpu().numpy() - (ref + bias_h)).max() / scale
    print("gemm_mx", M, N, K, "max rel err", err)
    assert err <= 1e-4
    h = _Guarded(M, N, torch.bfloat16)
    _gemm_ex(M, N, K, *ops, zero, bias=bias, ct=h.out)
    h.check("bf16 out")
    assert torch.equal(f.out.to(torch.bfloat16), h.out)
    # fc2 form: the bf16 residual stream read and rewritten in place = bf16(fp32 result + residual)
    res = dev(rng.standard_normal((M, N)).astype(np.float32)).to(torch.bfloat16)
    c = _Guarded(M, N, torch.bfloat16)
    c.out.copy_(res)
    _gemm_ex(M, N, K, *ops, zero, bias=bias, resid_t=c.out, ct=c.out)
    c.check("bf16 residual in place")
    want = ref + bias_h + res.float().cpu().numpy()
    got = c.out.float().cpu().numpy()
    assert np.abs(got - want).max() <= 1e-4 * scale + 2.0 ** -8 * np.abs(want).max()   # + the bf16 half-ulp
    assert torch.equal(c.out, (f.out + res.float()).to(torch.bfloat16))
    # fc1 form: bias, the fp8-out GELU polynomial (ACT_GELU_FAST), MX-fp8 out in the A layout of a GEMM with K = N --
    # restated from the GPU's own pre-activation at the bars of test_gemm_mx_fp8_output_is_the_quantised_result
    # (the two evaluations may straddle an e4m3 rounding boundary: >= 98 % of codes equal, >= 99.9 % within one
    # code, >= 99.5 % of scales equal)
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "..", "tools"))
    from fit_gelu import gelu_fast as gelu_poly
    coef = np.array([3.963519037e-01, -6.208017841e-02, 7.574830670e-03, -5.630472442e-04, 2.229058919e-05,
                     -3.503167250e-07])
    q = _Guarded(M, N, torch.uint8)
    sc = torch.zeros(mx_scale_bytes(M, N), dtype=torch.uint8, device="cuda")
    _gemm_ex(M, N, K, *ops, zero, bias=bias, ct=q.out, c_scale=sc, act=2)
    q.check("fp8 out")
    q0, _, e0 = mx.quantize(gelu_poly(f.out.cpu().numpy(), coef, 3.5), 0)
    qg = q.out.cpu().numpy().copy()
    qg[qg == 0x80] = 0   # -0 (tails past the clamp) equals +0
    q0 = q0.copy()
    q0[q0 == 0x80] = 0
    assert (qg == q0).mean() >= 0.98
    assert (np.abs(qg.astype(np.int16) - q0.astype(np.int16)) <= 1).mean() >= 0.999   # sign-magnitude codes
    assert (mx.exps_from_scales(sc.cpu().numpy(), M, N, 0) == e0).mean() >= 0.995


def test_post_ln_wavlm_is_refused(wavlm_sd):
    from ssr_amd import _lib, config as C
    from ssr_amd.hf import WavLMModel
    from ssr_amd.model import SSEModel
    for build in (lambda: SSEModel(C.WAVLM_BASE, wavlm_sd, device="cuda:0", dtype="fp8"),
                  lambda: WavLMModel.from_state_dict(C.WAVLM_BASE, wavlm_sd, device="cuda:0", dtype="fp8")):
        with pytest.raises(_lib.SSEError) as e:
            build()
        msg = str(e.value)
        assert "post-LN WavLM is not supported in fp8" in msg and "bf16" in msg and "fp16" in msg, msg


def test_no_state_leaks_into_bf16(sd, m8, bf16_before, fixture_clips):
    """A bf16 model built after an fp8 one (and after fp8 calls) embeds bit-identically to one built before."""
    m8.embed(fixture_clips, IDX)
    after = _model(sd, "bf16").embed(fixture_clips, IDX)
    assert torch.equal(after, bf16_before[1])
    assert torch.equal(bf16_before[0].embed(fixture_clips, IDX), bf16_before[1])


def test_drop_in_surface(m8, bf16_before, fixture_clips):
    """extract's in-memory twin and corpus.sse_embed_fn on an fp8 WavLM-large model: keys and shapes of the bf16 call."""
    from ssr_amd.corpus import sse_embed_fn
    from ssr_amd.extract import extract_embeddings_from_audio_wavlm
    from ssr_amd.hf import Wav2Vec2FeatureExtractor, WavLMModel
    fe = Wav2Vec2FeatureExtractor(do_normalize=False, device="cuda:0")
    clips = fixture_clips[:2].cpu().numpy()
    for clip in clips:
        d8 = extract_embeddings_from_audio_wavlm(clip, WavLMModel(m8), fe, "cuda:0", IDX)
        d16 = extract_embeddings_from_audio_wavlm(clip, WavLMModel(bf16_before[0]), fe, "cuda:0", IDX)
        assert d8 is not None and list(d8) == list(d16) == [f"layer_{i}" for i in IDX]
        for k in d8:
            assert d8[k].dtype == np.float32 and d8[k].shape == d16[k].shape == (1024,)
            assert np.isfinite(d8[k]).all()
    out = torch.empty((2, 4, 1024), device="cuda:0")
    got = sse_embed_fn(m8, IDX)(fixture_clips[:2], None, out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got, m8.embed(fixture_clips[:2], IDX))
