/*
 * adp_ar.h -- extension of adp.h: the elementwise math of autoregressive v-diffusion (the reference's ARVDiffusion and
 * ARVSampler, audio_diffusion_pytorch/diffusion.py:98-130 and :193-296).  Exported by the same libadp_hip.so.
 *
 * Conventions are adp.h's: plain fp32 device pointers that need the alignment of a float only (16-byte accesses are
 * chosen by looking at the pointers and at the split length, with a scalar path behind them), int64 sizes, a hipStream_t
 * passed as void*, 0 (ADP_OK) or a negative ADP_ERR_* code, no allocation, no synchronisation, hipGraph-capturable.
 *
 * A window of T positions is cut into N = num_splits splits of l = T / N positions; position t belongs to split t / l.
 * Every split has its own noise level sigma, and the net reads the levels as one extra input channel: the sigma plane,
 * [B, T] (= [B, 1, T]), which the depth-0 convs take through their second input pointer (adp_conv_desc.x2).
 * All three functions return ADP_ERR_SHAPE, and touch nothing, when T % N != 0 or a size is not positive.
 */
#ifndef ADP_AR_H
#define ADP_AR_H
#include "adp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ARVDiffusion.forward's noising (diffusion.py:118-127) in one pass.  sigma is [B, N]; per (batch, split)
 * a = cos((sigma * pi) / 2), b = sin(.) in fp32 (evaluated once per thread, not per element), then over [B, C, T]
 *   x_noisy = a x + b noise ; v_target = a noise - b x ; sigma_plane[b, t] = sigma[b, t / l]. */
int adp_arv_noise(const float* x, const float* noise, const float* sigma, int64_t B, int64_t C, int64_t T, int64_t N,
                  float* x_noisy, float* v_target, float* sigma_plane, void* stream);

/* One ARVSampler.sample_loop update (diffusion.py:231-235).  coef is device [N, 5]: row s = (a_i, b_i, a_{i+1}, b_{i+1},
 * sigma_{i+1}) of split s, the same for every batch row.
 *   x_out = a1 (a0 x - b0 v) + b1 (b0 x + a0 v)      (adp_v_step's operation order)
 * sigma_plane_out ([B, T], may be NULL) receives the NEXT step's plane: sigma_{i+1} of each position's split.
 * x_out may be x.  A split whose row is (1, 0, 1, 0, .) -- the context half of the ladder -- keeps its elements' values. */
int adp_arv_step(const float* x, const float* v, const float* coef, int64_t B, int64_t C, int64_t T, int64_t N,
                 float* x_out, float* sigma_plane_out, void* stream);

/* The first plane of a loop: sigma_plane[b, t] = sigma[t / l], sigma is [N]. */
int adp_arv_plane(const float* sigma, int64_t B, int64_t T, int64_t N, float* sigma_plane, void* stream);

#ifdef __cplusplus
}
#endif
#endif
