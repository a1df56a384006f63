/*
 * td_batch.h — C-ABI of the training-batch library (libtd_batch.so): the device half of the items the reference's three dataset classes build
 * one at a time on the CPU (terrain_diffusion/training/datasets/),
 *   H5LatentsDataset        h5_latents_dataset.py: the latent draw (:306-311), the lowfreq crop (:313-328), _get_cond_image (:149-224),
 *                           build_cond_inputs (:226-244),
 *   H5DecoderTerrainDataset h5_decoder_terrain_dataset.py: the lowfreq and residual crops (:196-228), the half-precision latent draw and its
 *                           nearest upsampling (:213-230),
 *   H5AutoencoderDataset    h5_autoencoder_dataset.py: the residual crop and its dihedral view (:166-196).
 * terrain_diffusion_amd/train_data.py holds the host halves: the key lists, the torch.Generator draws in the reference's order, the tables.
 *
 * Conventions as in td_coarse.h: a library of its own beside libtd_engine.so, plain C, a CALLER-SUPPLIED HIP stream (pass td_engine_stream),
 * device buffers only, synchronize = 0 only enqueues, synchronize = 1 completes on return; 0 on success / negative code with a message in
 * td_batch_last_error().  No call needs scratch.  Every result is independent of the order the device visits elements in: floating sums go
 * through a fixed tree, counters in LDS are integers, there is no floating-point atomic; two calls on the same inputs give the same bits.
 *
 * The planes stay resident.  A call names them through two device tables that are never read back:
 *   the GROUP table, td_batch_group[G]: the planes of one res/chunk/subchunk group and its side S (every plane of a group is square);
 *   the ITEM table, int32[N][TD_BATCH_ITEM_FIELDS]: group, i, j, transform_idx, li, lj -- the crop origin (i, j) the reference draws, the
 *   dihedral transform 0 .. 7, and the origin (li, lj) of the same crop in the untransformed plane, which the reference derives by undoing
 *   the transform (h5_latents_dataset.py:299-303).  An item whose group or transform is out of range gives NaN (views, cond image) or zeros
 *   (latents); a position outside its plane reads nothing.
 *
 * The dihedral VIEW of a window A is always flip(A, dims=[-1]) if transform_idx / 4 == 1, then rot90(., k = transform_idx % 4, dims=[-2, -1]).
 */
#ifndef TD_BATCH_H
#define TD_BATCH_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TD_BATCH_ITEM_FIELDS 6            /* group, i, j, transform_idx, li, lj */
#define TD_BATCH_MAX_ITEMS 65536          /* 1 <= N <= 65536 per call */
#define TD_BATCH_MAX_GROUPS 1048576       /* 1 <= G <= 2^20 */
#define TD_BATCH_MAX_CROP 4096            /* sides of an output window */
#define TD_BATCH_HALO 32                  /* the cond image: a halo of 32 pixels, blocks of 32 x 32 */
#define TD_BATCH_COND_CHANNELS 7          /* mean, p5, four climate means, mask */
#define TD_BATCH_COND_LEN 58              /* 16 + 16 + 4 + 16 + 5 + 1 */
#define TD_BATCH_PLANE_LOWFREQ 0
#define TD_BATCH_PLANE_LOWRES_EXACT 1
#define TD_BATCH_PLANE_RESIDUAL 2

typedef struct td_batch_group {
    const void* latent;          /* fp16 (8, 2 lc, S, S): one slab per transform, means then logvars; may be null where no call reads it */
    const float* lowfreq;        /* fp32 (S, S) */
    const float* lowres_exact;   /* fp32 (S, S) */
    const float* climate;        /* fp32 (4, S, S): the channels 0, 3, 11, 14 of the group's climate, in that order */
    const float* residual;       /* fp32 (R, R), R = 8 S for the reference's data */
    int32_t side;                /* S */
    int32_t residual_side;       /* R */
} td_batch_group;

const char* td_batch_last_error(void);

/* out (N, h, w) fp32: out[n] is the dihedral view of a window of plane `plane` (TD_BATCH_PLANE_*) of item n's group.  The window is
 * (h, w) for an even rotation and (w, h) for an odd one, so that the view is (h, w); its first row and column are
 *   origin = 0: (li + offset, lj + offset)   the reference's inverse offsets: lowfreq, lowfreq_padded (offset -1, h = crop + 2), residual;
 *   origin = 1: (i + offset, j + offset)     the window itself: the decoder's lowfreq, the autoencoder's crop.
 * Positions outside the plane are NaN (the reference's np.full(nan) placement).  affine = 1 applies ((x - a) / b) * c in fp32, three
 * rounded operations in that order: the reference's `(x - a) / b * c` of lowfreq and its `(x - a) / b` followed by `* c` of the decoder's
 * residual are both this sequence; c = 1 leaves the quotient.  affine = 0 copies.  1 <= h, w <= 4096, |offset| <= 4096. */
int td_batch_views(void* hip_stream, const td_batch_group* groups, int G, const int32_t* items, int N, int plane, int origin, int offset,
                   int h, int w, int affine, float a, float b, float c, float* out, int synchronize);

/* The reparameterisation from slab transform_idx of the group's latent: means m = latent[t, ch, i + r, j + q], logvars
 * v = latent[t, lc + ch, ...], e = fp16(exp(fp16(0.5 v))) with the exponential rounded once to half.
 *   mode 0 (h5_latents_dataset.py:306-311): noise fp32 (N, lc, h, w); out fp32 (N, lc, h, w) = ((n e + m) - mean[ch]) / std[ch] * sigma_data,
 *           every operation in fp32 on the promoted halves;
 *   mode 1 (h5_decoder_terrain_dataset.py:213-230): noise fp16 (N, lc, h, w); out fp16 (N, lc, 8 h, 8 w) = fp16(fp16(n e) + m) -- each
 *           operation carried out in fp32 on the promoted halves and rounded to half, as torch's CPU kernels do -- repeated over 8 x 8
 *           pixels (F.interpolate(mode='nearest')); mean, std and sigma_data are not read.
 * A position outside the latent reads nothing and gives 0.  mean, std: device fp32 (lc).  1 <= lc <= 64, 1 <= h, w <= 4096. */
int td_batch_latents(void* hip_stream, const td_batch_group* groups, int G, const int32_t* items, int N, int lc, int h, int w, int mode,
                     const void* noise, const float* mean, const float* std, float sigma_data, void* out, int synchronize);

/* out (N, 7, g, g) fp32, g = (crop + 64) / 32: _get_cond_image (h5_latents_dataset.py:149-224) of the window of `crop` pixels at (li, lj)
 * with its halo of 32, read straight from lowres_exact and the four climate planes through the inverse of the view; the haloed window is
 * never written.  Per 32 x 32 block of the VIEW:
 *   mean     the float64 sum of the 1024 values through a fixed tree, divided by 1024, rounded once to fp32; a NaN or a position outside the
 *            plane gives NaN (channel 0; channels 2 .. 5 likewise for the climate planes);
 *   p5       numpy's `linear` 0.05 quantile as numpy computes it for fp32 input, all in fp32: r = fl(1023) fl(0.05), k = floor(r),
 *            t = fl(r - k), a + (b - a) t over the exact order statistics k and k + 1 (an exact radix select over order-preserving integer
 *            keys); NaN where the mean is NaN (channel 1);
 *   mask     1 - isnan(mean) (channel 6);
 *   dropout  u_drop (N, g, g) non-null: mask *= (u_drop > dropout_p), mean and p5 become NaN where the mask is 0;
 *   noise    u_noise (N) non-null: mean += z_mean s and p5 += z_p5 s with s = fl(u_noise[n] max_noise), z_mean, z_p5 (N, g, g) normals;
 *   raw = 0: mean and p5 go through nan_to_num (NaN -> norm_mean[0], norm_mean[1]; +-inf -> +-FLT_MAX), then every channel is
 *            (x - norm_mean[ch]) / norm_std[ch] in fp32; climate NaNs stay NaN.  raw = 1 leaves the stack as it is (the reference's
 *            `cond_input_mean is None` branch); norm_mean and norm_std are not read.
 * crop a multiple of 32, 64 <= crop <= 4096.  norm_mean, norm_std: device fp32 (7). */
int td_batch_cond_image(void* hip_stream, const td_batch_group* groups, int G, const int32_t* items, int N, int crop, float dropout_p,
                        const float* u_drop, float max_noise, const float* u_noise, const float* z_mean, const float* z_p5,
                        const float* norm_mean, const float* norm_std, int raw, float* out, int synchronize);

/* out (N, 58) fp32: build_cond_inputs (h5_latents_dataset.py:226-244) of cond_img (N, 7, g, g), g >= 4, with c = g / 2:
 *   [0, 16)   cond_img[0, c - 2 : c + 2, c - 2 : c + 2] row-major, times factors[0];      [16, 32)  channel 1, times factors[1];
 *   [32, 36)  the means ((x00 + x01) + x10) + x11) / 4 of the 2 x 2 centre of channels 2 .. 5, a NaN mean replaced by z_replace[n][slot],
 *             times factors[2];                                                           [36, 52)  channel 6, times factors[3];
 *   [52, 57)  histogram_raw[n], times factors[4];                                         [57]      fl(fl(noise_level[n] - 0.5) sqrt12) times factors[5].
 * factors (6 fp32, host values passed by value through f0 .. f5) are mp_concat's per-part scales.  nan_flags (N, 4) int32 receives 1 where
 * the climate mean was NaN, else 0.  z_replace may be null: NaN means then stay (the caller reads the flags first). */
int td_batch_cond_vector(void* hip_stream, const float* cond_img, int N, int g, const float* histogram_raw, const float* noise_level,
                         const float* z_replace, float sqrt12, float f0, float f1, float f2, float f3, float f4, float f5, float* out,
                         int32_t* nan_flags, int synchronize);

#ifdef __cplusplus
}
#endif
#endif
