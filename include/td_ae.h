/*
 * td_ae.h -- the autoencoder entry points of libtd_engine.so (part of the C-ABI of include/td_engine.h, which includes this file; including
 * either header declares everything).  Same conventions as td_engine.h: plain C, opaque handles, 0 / negative code with td_last_error(),
 * pointers host or device unless said otherwise.
 */
#ifndef TD_AE_H
#define TD_AE_H
#include "td_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- autoencoder --------------------------------------------------------------------------------------------
 * Replaces EDMAutoencoder(...) + load_state_dict (terrain_diffusion/models/edm_autoencoder.py:13-158): the model that turns real elevation into the
 * base model's latent space and back.  Its two stacks run on the U-Net's block machinery as two further graph kinds: an encoder-only stack whose
 * out_conv sits on the bottleneck (edm_unet.py:107-139 with encode_only=True) and a skip-less decoder behind a 1x1 decoder_conv
 * (edm_autoencoder.py:86-103); neither has an embedding (emb_channels = 0: a block's epilogue is mp_silu(y), unet_block.py:133-134).
 * td_ae_config: the constructor arguments of edm_autoencoder.py:15-32 that shape the graph.  Limits (TD_ERR_UNSUPPORTED): latent_channels <= 4,
 * latent_channels + n_direct_skips + 1 <= 32, in_channels + 1 <= 32, out_channels <= 8, block channels multiples of 64; conditional_inputs and
 * block_kwargs are not carried. */
typedef struct td_ae td_ae;
typedef struct td_ae_config {
    int32_t image_size;            /* block names / attention resolution test only */
    int32_t in_channels, out_channels;
    int32_t model_channels;
    int32_t n_levels;
    int32_t channel_mults[8];
    int32_t layers_per_block[8];
    int32_t layers_per_block_decoder[8];
    int32_t n_attn_resolutions;
    int32_t attn_resolutions[8];
    int32_t midblock_attention;
    int32_t latent_channels;
    int32_t n_direct_skips;
    int32_t direct_skips[8];
} td_ae_config;
int td_ae_create(td_engine* e, const td_ae_config* cfg, int dtype, td_ae** out);
void td_ae_destroy(td_ae* ae);
/* Parameters under the reference's state-dict names ("encoder.enc.<res>x<res>_block<i>.conv_res0.weight", "encoder.out_conv.weight",
 * "encoder.out_gain", "decoder_conv.weight", "decoder.<i>.conv_res1.weight", "out_conv.weight", "out_gain", ...), with the semantics of their
 * td_unet_* twins (raw weights folded here in fp64, or prefolded by the host).  td_ae_set_param accepts and ignores what the state dict holds and
 * inference never reads: "*.emb_gain" (unet_block.py:72, unused without an embedding), "logvar", "encoder.logvar_*". */
int td_ae_num_params(td_ae* ae);
int td_ae_param_info(td_ae* ae, int i, const char** name, int32_t* ndim, int64_t shape[4]);
int td_ae_set_param(td_ae* ae, const char* name, const float* host_data, int64_t numel);
int td_ae_set_prefolded(td_ae* ae, int prefolded);
int td_ae_finalize(td_ae* ae);
/* EDMAutoencoder.preencode (edm_autoencoder.py:107-123) of (x - mean) / std, x: [n_src][in_channels][H][W] fp32; one subtraction and one true division
 * in fp32, as build_encoded_dataset.py:69 executes them (mean = 0, std = 1: x itself).  dihedral = 0: one image per source; 1: the 8 views of
 * build_encoded_dataset.py:75-81 per source, image 4 * flip + r = rot90(flip(x, [-1]) if flip else x, k = r), H == W -- the loop body of
 * build_encoded_dataset.py:68-94 for one chunk as ONE batch.  With n = n_src or 8 * n_src, L = latent_channels, D = n_direct_skips, h = H / 2^(levels-1):
 * means, logvars: [n][L + D][h][w] fp32.  Direct channel d of means = mean of the 2^(levels-1)-square blocks of input channel direct_skips[d], from the
 * fp32 source (never the 16-bit staged input); of logvars, -20.  packed_f16 (may be NULL): [n][2 (L + D)][h][w] binary16 = cat(means, logvars) rounded
 * to nearest even, the dataset's storage form (:87,94).  H, W divisible by 2^(levels-1).  Host or device pointers; enqueue-only under "async" when
 * all are device pointers. */
int td_ae_preencode(td_ae* ae, int n_src, int H, int W, const float* x, float mean, float std, int dihedral, float* means, float* logvars, void* packed_f16);
/* EDMAutoencoder.postencode (edm_autoencoder.py:125-130) with the caller's noise: z = means + eps * exp(0.5 * logvars) over numel elements (the
 * reference draws eps = randn_like; here it is an argument, e.g. td_standard_normal).  Host or device; enqueue-only under "async" for device pointers. */
int td_ae_postencode(td_ae* ae, int64_t numel, const float* means, const float* logvars, const float* eps, float* z);
/* EDMAutoencoder.decode (edm_autoencoder.py:132-158): z [n][L + D][h][w] -> out [n][out_channels][h 2^(levels-1)][w 2^(levels-1)]; output channel
 * direct_skips[d] is the nearest-neighbour upsampling of latent channel L + d.  Then out * std + mean (a multiply and an add, rounded separately, as
 * torch's `y * std + mean`); std = 1 with mean = 0 leaves the decoder's output as it is.  Host or device; enqueue-only under "async" for device pointers. */
int td_ae_decode(td_ae* ae, int n, int h, int w, const float* z, float std, float mean, float* out);
/* Test facility: td_unet_read_activation on one of the two stacks, as the last td_ae_preencode (stack 1, the encoder) or td_ae_decode (stack 2, the
 * decoder) of that batch and map left it.  H, W: that stack's own input map, the image for the encoder (n = 8 * n_src in the dihedral form), the
 * latent for the decoder.  label: a conv or attention op's profile label, "sumsq:<label>", or "@xin" (the staged NHWC input, every channel of its
 * K chunk).  The labels of what these stacks do not have -- "@emb", "@cvec", "@emb:rows", "@cvec:rows" (no embedding: the modulation is one shared row
 * of ones) and "@x", "@m1", "@m2", "@xt" (no sampler state) -- are refused with TD_ERR_ARG, as is any other stack.  Always waits for the stream. */
int td_ae_read_activation(td_ae* ae, int stack, int n, int H, int W, const char* label, float* out_host, int64_t capacity, int32_t dims[4]);

#ifdef __cplusplus
}
#endif
#endif
