#pragma once
#include "common.h"

constexpr int LM_NFFT = 400;   // Whisper STFT: 400-point frames, hop 160, 201 bins
constexpr int LM_MAXMEL = 128;   // n_mels: 80 (v1/v2) or 128 (v3)

constexpr int LM_NFR = 3000;     // mel frames of the 30 s pad (two per encoder frame)

// nfr: mel frames computed per clip, even, 2 .. LM_NFR (a Whisper audio context of F encoder frames: 2 F)
size_t logmel_workspace_bytes(int B, int n_mels, int nfr = LM_NFR);
// x [B][L] fp32 -> out_hf [B][n_mels][nfr] fp32 (optional) and out_cl [B][nfr][n_mels] (optional): the first nfr
// frames of the log-mel of the clip cut at 160 nfr samples (the per-clip max of the -8 clamp over those frames);
// lens (ragged batch, device, optional): samples of each clip, zeros after (the feature extractor's padding)
template <typename TO>
int launch_logmel(const float* x, int B, int L, int n_mels, int nfr, float* out_hf, TO* out_cl, void* ws,
                  size_t ws_bytes, hipStream_t s, const int* lens = nullptr);
// HF-layout mel [B][n_mels][nfr] fp32 -> channels-last [B][nfr][n_mels]
template <typename TO>
int launch_mel_to_cl(const float* mel_hf, int B, int n_mels, int nfr, TO* out_cl, hipStream_t s);
// y = (x - st[b].mean) * st[b].rstd
int launch_normalize_apply(const float* x, int B, int L, const float* st, float* y, hipStream_t s);
