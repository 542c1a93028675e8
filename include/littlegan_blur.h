/* littlegan_blur.h — a faded Gaussian blur of every image the Discriminator reads (blur_init_sigma, blur_fade_kimg), no counterpart
 * in the reference.
 *
 * Entry points with the `lgblur_` prefix, exported by liblittlegan_hip.so under the conventions of littlegan_hip_ext.h — plain C, device
 * pointers, fp32, `stream` a hipStream_t passed as void* (NULL = default stream), return LG_OK (0) or LG_ERR_* with the message in
 * lg_last_error(), no allocation, no synchronisation, no atomics, every argument checked on the host before any launch, every launch
 * noted for lg_last_kernel().  lg_abi_version() stays 1: nothing declared in littlegan_hip*.h changes.  (Part of the C ABI like every
 * include/littlegan_*.h: bound by _lib.SIGNATURES, held to it by tests/test_abi.py.)
 *
 * ---- the definition (THIS PROJECT's; the filter is the discriminator-input blur of Karras et al. 2021, "Alias-free GANs") ---------- *
 * Images: x[rows][S][S][3] fp32 NHWC, S % 8 == 0, 8 <= S <= 1024 (lgeo_fwd's limits).
 * Schedule: k = the training steps taken before this one, n = the real images D reads per step over all ranks, F = the images over which
 * the blur fades.  In fp64, with basic operations only (host and device agree bit for bit):
 *     sigma64 = sigma0 * max(1 - (double)(k n) / (double)F, 0)        sigma = (float)sigma64
 *     R       = min((int)floorf(3.0f * sigma), 30);  a sigma that is not finite or not > 0 gives R = 0
 * lgblur_apply derives R from sigma itself: sigma is the only word it reads.
 * Taps, for R >= 1:  t_i = exp2(-(i / sigma)^2) in fp64, i = 0..R;  Z = t_0 + 2 (t_1 + ... + t_R), summed in ascending i;
 *     w_i = (float)(t_i / Z)
 * Operator:
 *     h(y, x)   = sum over i = -R..R, ascending, of w_|i| x(y, x + i)
 *     out(y, x) = sum over j = -R..R, ascending, of w_|j| h(y + j, x)
 * per channel, fp32, every sum started from +0, one rounding per operation (the library is built with -ffp-contract=off).  A tap outside
 * the image contributes nothing and is not read (zero fill, no renormalisation: filter2d's zero padding, and this project's other
 * transforms).  R == 0 returns x bit for bit.  The bits of an output pixel depend on its image, sigma and S only: not on the row's place
 * in the batch, the batch size, the tile geometry or the launch.
 * Adjoint: H and V are symmetric under zero fill, so Blur^T is Blur up to rounding: the backward pass is lgblur_apply on the gradient.
 * config.py::blur_restate restates the schedule and the taps on the host in numpy.
 *
 * ---- the state: 16 bytes of device memory, 16-byte aligned ----------------------------------------------------------------------- *
 *     word 0      int32  k: the steps lgblur_step has taken, saturating at 2^31 - 1
 *     word 1      fp32   sigma of the most recent lgblur_step (0 after lgblur_init)
 *     words 2, 3  zero */
#ifndef DBLUR_H
#define DBLUR_H

#ifdef __cplusplus
extern "C" {
#endif

#define DBLUR_MAX_RADIUS 30

/* state = {k0, 0.f, 0, 0}, written by one thread from the launch scalar: no host-to-device copy.  0 <= k0 < 2^31. */
int lgblur_init(float* state, long long k0, void* stream);

/* state word 1 = sigma(k) by the definition above with k = word 0 (a negative k counts as 0), then k += 1, saturating.  sigma0 finite
 * and >= 0; 1 <= images_per_step <= 2^31; 1 <= fade_images <= 2^40.  One launch, one thread.  The first of the blur's launches in a step. */
int lgblur_step(float* state, float sigma0, long long images_per_step, long long fade_images, void* stream);

/* out[rows][S][S][3] = Blur(x) under state word 1.  x, state, out 16-byte aligned, x != out, 1 <= rows <= 2^20.  One launch, no
 * workspace.  For ANY state bits no access leaves the images (NaN, Inf, a negative or a huge sigma included: R is clamped to 0..30).
 * A row range of a batch gives the bits it has in the whole batch.  Serves the forward and the adjoint. */
int lgblur_apply(const float* x, const float* state, float* out, int rows, int S, void* stream);

#ifdef __cplusplus
}
#endif
#endif
