// The C ABI of libpiamd_kernels.so: every exported entry point, declared once.
//   * common.h includes this header, so a definition in csrc/kernels/*.hip that disagrees with its
//     declaration does not compile (C-linkage functions cannot be overloaded).
//   * ops/_lib.py parses it at load time for the ctypes argtypes / restype and refuses a library
//     that lacks a declared symbol. Keep to `PIAMD_EXPORT <ret> piamd_<name>(<type> <name>, ...);`
//     with int, float, long long, uint64_t, hipStream_t and pointers.
//   * the native engine (csrc/native) includes it instead of copying prototypes.
// Launchers return the hipError_t of their launch as int and take the stream last. The argument
// contract of an entry point is the comment above its definition in the file named here. One name
// per entry point: a new argument goes into the declaration and every caller, not a suffixed copy.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "decode_args.h"
#include "fa_args.h"

#define PIAMD_EXPORT extern "C" __attribute__((visibility("default")))

// ---- agemm_host.hip (the assembly GEMM; colsum nullable)
PIAMD_EXPORT int piamd_agemm_load(const char* path);
PIAMD_EXPORT int piamd_agemm(const void* a, long long lda, int trans_a, const void* b,
    long long ldb, int trans_b, void* c, long long ldc, int c_f32, int accumulate, int M, int N,
    int K, int epi, int act, const void* bias, void* aux, long long ldaux, int ksplit, void* ws,
    int f16, int batch, long long sa, long long sb, long long sc, void* colsum, hipStream_t st);

// ---- batchnorm.hip
PIAMD_EXPORT int piamd_bn_set_parts(long long elems_per_block, int max_parts);
PIAMD_EXPORT int piamd_bn_fwd(int dtype, int nhwc, const void* x, const void* res, void* y, int N,
    int C, int S, const float* gamma, const float* beta, float* run_mean, float* run_var,
    float* mean, float* rstd, float momentum, float eps, int training, int act, float* ws,
    float* ss, const float* part_t, int P_t, hipStream_t st);
PIAMD_EXPORT int piamd_bn_bwd(int dtype, int nhwc, const void* dy, const void* y, const void* x,
    void* dx, void* dres, int N, int C, int S, const float* gamma, const float* mean,
    const float* rstd, float* dgamma, float* dbeta, int training, int act, float* ws,
    const float* ss, hipStream_t st);
PIAMD_EXPORT int piamd_bn_local_stats(int dtype, int nhwc, const void* x, int N, int C, int S,
    float* ws, float* out, hipStream_t st);
PIAMD_EXPORT int piamd_bn_bwd_local_sums(int dtype, int nhwc, const void* dy, const void* y,
    const void* x, int N, int C, int S, const float* mean, const float* rstd, int act, float* ws,
    const float* ss, float* out, hipStream_t st);
PIAMD_EXPORT int piamd_bn_bwd_apply_sums(int dtype, int nhwc, const void* dy, const void* y,
    const void* x, void* dx, void* dres, int N, int C, int S, const float* gamma, const float* mean,
    const float* rstd, int act, const float* sums, float Mtot, float* ws, const float* ss,
    hipStream_t st);

// ---- conv_dw.hip
PIAMD_EXPORT int piamd_dconv2d(const void* in, const void* w, const void* bias, void* out, int N,
    int H, int W, int Cin, int OH, int OW, int Cout, int R, int S, int st_h, int st_w, int pad_h,
    int pad_w, int dil_h, int dil_w, int cin_g, int cout_g, int transposed, int dtype,
    hipStream_t st);
PIAMD_EXPORT long long piamd_dconv2d_wgrad_parts(int N, int H, int W, int C, int OH, int OW, int K,
    int R, int S, int st_h, int st_w, int pad_h, int pad_w, int dil_h, int dil_w, int cin_g,
    int cout_g, int dtype);
PIAMD_EXPORT int piamd_dconv2d_wgrad(const void* x, const void* dy, float* d, float* ws, int parts,
    int N, int H, int W, int Cin, int OH, int OW, int Cout, int R, int S, int st_h, int st_w,
    int pad_h, int pad_w, int dil_h, int dil_w, int cin_g, int cout_g, int dtype, hipStream_t st);

// ---- conv_wprep.hip
PIAMD_EXPORT int piamd_conv_wprep(int src_dt, int f16, const void* w, void* fwd, void* dgr, int K0,
    int C0, int R, int S, int K4, int Cp, int Kp, hipStream_t st);

// ---- debug.hip: *flag = min(*flag, op_id) if x (dtype 0 f32, 1 bf16, 2 fp16) holds a NaN or Inf
PIAMD_EXPORT int piamd_nan_inf_check(int dtype, const void* x, long long n, int* flag, int op_id,
    hipStream_t st);

// ---- decode_mega.hip (argument blocks: decode_args.h)
PIAMD_EXPORT int piamd_decode_mega_variant_supported(int E_, int D_, int hq, int hk, int F_,
    int rot, int w8, int nb, int mm);
PIAMD_EXPORT int piamd_decode_mega_batch_supported(int E_, int D_, int hq, int hk, int F_, int rot,
    int w8, int nb);
PIAMD_EXPORT int piamd_decode_mega_shape_supported(int E_, int D_, int hq, int hk, int F_, int rot,
    int w8);
PIAMD_EXPORT int piamd_decode_mega(const MegaArgs* args, int E_, int D_, int hq, int hk, int F_,
    hipStream_t st);
PIAMD_EXPORT int piamd_decode_head_greedy(const HeadArgs* args, int E_, hipStream_t st);

// ---- elementwise.hip (piamd_f32_split_hilo: contract above split3_f32_kernel)
PIAMD_EXPORT int piamd_bias_act_fwd(int dt, int act, const void* x, const void* bias, void* y,
    void* pre, long long n, int N, hipStream_t stream);
PIAMD_EXPORT int piamd_bias_act_bwd(int dt, int act, const void* dy, const void* h,
    const void* bias, void* dx, void* dbias, float* part, int rows, int N, int accumulate,
    hipStream_t stream);
PIAMD_EXPORT int piamd_softmax_fwd(int dt, const void* x, const void* mask, int mask_rows,
    int causal_q, void* y, int rows, int N, float scale, hipStream_t stream);
PIAMD_EXPORT int piamd_softmax_bwd(int dt, const void* y, const void* dy, void* dx, int rows, int N,
    float scale, hipStream_t stream);
PIAMD_EXPORT int piamd_dropout(int dt, const void* x, void* y, long long n, float p, uint64_t seed,
    uint64_t offset, hipStream_t stream);
PIAMD_EXPORT int piamd_bf16_transpose(const void* src, void* dst, int R, int C, hipStream_t stream);
PIAMD_EXPORT int piamd_f32_split_hilo(const void* src, long long ld, void* dst, int R, int C,
    int Rp, int Cp, int lo_mask, int axis, hipStream_t stream);

// ---- embedding.hip: the _dt backward takes any dy dtype into an f32 dW, the other a bf16 dy into a
// bf16 or f32 dW (different kernels)
PIAMD_EXPORT int piamd_embedding_fwd(int dtype, const long long* ids, const void* w,
    long long start, int vlocal, const void* p, const long long* pos, int S, void* out, long long T,
    int H, hipStream_t st);
PIAMD_EXPORT int piamd_embedding_bwd_dt(int dtype, const long long* sorted, const long long* order,
    const void* dy, float* dw, long long start, int vlocal, long long T, int H, int accumulate,
    hipStream_t st);
PIAMD_EXPORT int piamd_embedding_bwd(const long long* sorted, const long long* order,
    const void* dy, void* dw, int dw_f32, long long start, int vlocal, long long T, int H,
    int accumulate, hipStream_t st);
PIAMD_EXPORT int piamd_pos_embedding_bwd(const void* dy, void* dp, int dp_f32, int B, int S, int H,
    int accumulate, hipStream_t st);

// ---- fa_asm_host.hip
PIAMD_EXPORT int piamd_fa_asm_load(const char* path);
PIAMD_EXPORT int piamd_fa_asm_loaded();
PIAMD_EXPORT int piamd_fa_asm_enable(int mask);
PIAMD_EXPORT int piamd_fa_fwd_nw(int nw);
PIAMD_EXPORT int piamd_fa_asm_applies(const FaArgs* ap);

// ---- fft.hip
PIAMD_EXPORT int piamd_fft_c2c(const void* in, void* out, long long rows, int N, int inverse,
    float scale, hipStream_t st);

// ---- flash_attn.hip (argument block: fa_args.h; f16: fp16 operands, else bf16)
PIAMD_EXPORT int piamd_fa_fwd(const FaArgs* args, int f16, hipStream_t stream);
PIAMD_EXPORT int piamd_fa_bwd(const FaArgs* args, int f16, hipStream_t stream);

// ---- gemm.hip (piamd_conv2d_fwd: flags bit 0 = fp16; stats nullable; dst_h = 0: plain output)
PIAMD_EXPORT int piamd_int8_gemm(const void* x, long long ldx, const void* wq, long long ldw,
    const float* xs, float xs_const, const float* ws, const void* bias, void* y, long long ldy,
    int M, int N, int K, int act, hipStream_t st);
PIAMD_EXPORT int piamd_conv2d_fwd(const void* x, const void* wt, const void* zero, void* y, int N,
    int H, int W, int C, int OH, int OW, int R, int S, int st_h, int st_w, int pad_h, int pad_w,
    int dil_h, int dil_w, int Kout, int act, const void* bias, int tile_n, int ksplit, void* ws,
    int flags, float* stats, int dst_h, int dst_w, int rs_h, int rs_w, int ph, int pw,
    hipStream_t st);
PIAMD_EXPORT int piamd_conv2d_wgrad(const void* x, const void* dy, const void* zero, float* d,
    int N, int H, int W, int C, int OH, int OW, int R, int S, int st_h, int st_w, int pad_h,
    int pad_w, int dil_h, int dil_w, int Kout, int tile_n, int ksplit, float* ws, int accumulate,
    int f16, hipStream_t st);
PIAMD_EXPORT int piamd_quant_rows(const void* x, long long ldx, void* q, long long ldq,
    float* scale, float s_static, int M, int K, hipStream_t st);
PIAMD_EXPORT int piamd_moe_gemm(const void* x, long long ldx, const void* w, long long ldw,
    long long sw, int trans_w, const int* offs, int E, int rows_cap, void* y, long long ldy,
    int y_f32, int N, int K, int epi, int act, const void* bias, void* aux, long long ldaux,
    hipStream_t st);
PIAMD_EXPORT int piamd_moe_wgrad(const void* x, long long ldx, const void* dy, long long lddy,
    const int* offs, int E, void* dw, long long sdw, int dw_f32, int accumulate, int M, int N,
    hipStream_t st);

// ---- gemm_small.hip (every ln_* / rln_* pointer nullable: no LayerNorm fold)
PIAMD_EXPORT int piamd_small_gemm(int f16, const void* a, long long lda, const void* b,
    long long ldb, void* c, long long ldc, int c_f32, int M, int N, int K, int mb, int nb, int wn,
    int depth, int ks, float alpha, const void* bias, int act, const void* resid, long long ldr,
    float* ws, int* cnt, const float* ln_c1, const float* ln_b2, float ln_eps, float* ln_stats,
    const float* rln_stats, const void* rln_g, const void* rln_b, hipStream_t st);

// ---- groupnorm.hip
PIAMD_EXPORT int piamd_group_norm_fwd(int dtype, const void* x, void* y, const float* gamma,
    const float* beta, float* mean, float* rstd, float* ws, int N, int C, long long HW, int G,
    float eps, hipStream_t st);
PIAMD_EXPORT int piamd_group_norm_bwd(int dtype, const void* dy, const void* x, const float* gamma,
    const float* mean, const float* rstd, void* dx, float* dgamma, float* dbeta, float* ws, int N,
    int C, long long HW, int G, hipStream_t st);
PIAMD_EXPORT int piamd_group_norm_apply(int dtype, const void* x, void* y, const float* gamma,
    const float* beta, const float* mean, const float* rstd, int N, int C, long long HW, int G,
    hipStream_t st);

// ---- infer.hip (piamd_wo_gemm: ln_g / ln_b / resid nullable)
PIAMD_EXPORT int piamd_qkv_prep(void* qkv, long long ld, const void* bias, void* kc, void* vc,
    const int* pos0, int B, int S, int Hq, int Hk, int D, int maxS, int rot, int neox, float base,
    hipStream_t st);
PIAMD_EXPORT int piamd_decode_attn(const void* qkv, long long ldq, const void* bias, int prep,
    int rot, int neox, float base, void* kc, void* vc, const int* lens, int B, int Hq, int Hk,
    int D, int maxS, int chunk, int nsplit, const void* mask, long long ldm, float scale,
    float* part, int* cnt, void* out, long long ldo, hipStream_t st);
PIAMD_EXPORT int piamd_wo_gemm(int bits, const void* x, long long ldx, const void* wp,
    const float* scale, const void* bias, void* y, long long ldy, float* ws, int* cnt, int M, int N,
    int K, int KS, int act, const void* ln_g, const void* ln_b, float eps, const void* resid,
    long long ldr, hipStream_t st);
PIAMD_EXPORT int piamd_wo_moe_gemm(int bits, const void* x, long long ldx, const void* wp,
    long long wstride, const float* scale, const void* bias, const int* offs, int E, int rows_cap,
    void* y, long long ldy, int N, int K, int act, hipStream_t st);
PIAMD_EXPORT int piamd_wo_dequant(int bits, const void* wp, const float* scale, void* out, int N,
    int K, hipStream_t st);

// ---- layernorm.hip (flags bit 0 = RMSNorm). piamd_colsum: out [N] (+)= the column sums of x [rows][N]
// through the partials part f32 [G][N]
PIAMD_EXPORT int piamd_layernorm_fwd(int dtype, const void* x, const void* bias,
    const void* residual, const void* gamma, const void* beta, void* y, void* residual_out,
    float* mean, float* rstd, int rows, int N, float eps, float p_drop, uint64_t seed,
    uint64_t offset, int flags, hipStream_t stream);
PIAMD_EXPORT long long piamd_layernorm_bwd_ws(int rows, int N);
PIAMD_EXPORT int piamd_layernorm_bwd(int dtype, const void* dy, const void* h, const void* gamma,
    const float* mean, const float* rstd, const void* dres_in, void* dres, void* dx, void* dgamma,
    void* dbeta, void* dbias, float* ws, int rows, int N, float p_drop, uint64_t seed,
    uint64_t offset, int accum_mask, int flags, hipStream_t stream);
PIAMD_EXPORT int piamd_colsum(int dtype, const void* x, void* out, float* part, int G, int rows,
    int N, int accumulate, hipStream_t stream);
PIAMD_EXPORT int piamd_colsum_parts(int dtype, const float* part, int G, int N, void* out,
    int accumulate, hipStream_t stream);

// ---- optim.hip
PIAMD_EXPORT int piamd_adamw_flat(float* p, float* m, float* v, const void* grad, int grad_dtype,
    void* model, long long n, float lr, const float* lr_ptr, float beta1, float beta2, float eps,
    float wd, float bc1, float bc2_sqrt, const float* grad_scale, float static_grad_scale,
    hipStream_t stream);
PIAMD_EXPORT int piamd_momentum_flat(float* p, float* vel, const void* grad, int grad_dtype,
    void* model, long long n, float lr, const float* lr_ptr, float mu, float wd, int nesterov,
    const float* grad_scale, hipStream_t stream);
PIAMD_EXPORT int piamd_sumsq(const void* x, int dtype, long long n, float* partial, float* out,
    int accumulate, hipStream_t stream);
PIAMD_EXPORT int piamd_multi_tensor_update(int op, const long long* meta, const float* fmeta,
    const int* chunk_off, int T, int total_chunks, float lr, float mu, int nesterov, float beta1,
    float beta2, float eps, float bc1, float bc2_sqrt, const float* grad_scale, hipStream_t stream);

// ---- pool.hip
PIAMD_EXPORT int piamd_maxpool_fwd_nhwc(const void* x, void* y, void* idx, int N, int H, int W,
    int C, int OH, int OW, int kh, int kw, int sh, int sw, int ph, int pw, int f16, hipStream_t st);
PIAMD_EXPORT int piamd_maxpool_bwd_nhwc(const void* dy, const void* idx, void* dx, int N, int H,
    int W, int C, int OH, int OW, int kh, int kw, int sh, int sw, int ph, int pw, int f16,
    hipStream_t st);

// ---- pool_nd.hip: I / O / K / S / P and the interpolation's scale are HOST arrays of 3 values
// [D, H, W], read during the call; the interp / grid_sample backward write f32 gradients
PIAMD_EXPORT int piamd_pool_nd_fwd(int dt, const void* x, void* y, int* idx, int N, int C,
    const int* I, const int* O, const int* K, const int* S, const int* P, int mode, int adaptive,
    int exclusive, int divisor, hipStream_t st);
PIAMD_EXPORT int piamd_pool_nd_bwd(int dt, const void* dy, const int* idx, void* dx, int N, int C,
    const int* I, const int* O, const int* K, const int* S, const int* P, int mode, int adaptive,
    int exclusive, int divisor, hipStream_t st);
PIAMD_EXPORT int piamd_interp_fwd(int dt, const void* x, void* y, int N, int C, const int* I,
    const int* O, const float* scale, int mode, int align_corners, hipStream_t st);
PIAMD_EXPORT int piamd_interp_bwd(int dt, const void* dy, float* dx, int N, int C, const int* I,
    const int* O, const float* scale, int mode, int align_corners, hipStream_t st);
PIAMD_EXPORT int piamd_grid_sample_fwd(int dt, const void* x, const void* grid, void* y, int N,
    int C, int IH, int IW, int OH, int OW, int mode, int pad, int align_corners, hipStream_t st);
PIAMD_EXPORT int piamd_grid_sample_bwd(int dt, const void* dy, const void* x, const void* grid,
    float* dx, float* dgrid, int N, int C, int IH, int IW, int OH, int OW, int mode, int pad,
    int align_corners, hipStream_t st);

// ---- search.hip
PIAMD_EXPORT int piamd_beam_search_softmax(const void* logits, int logits_bf16, const float* cum,
    const int* seq_lens, const unsigned char* stop, const int* end_ids, const int* step_ids,
    const int* last_cache_ids, const int* last_beam_offsets, int bs, int beam, int V,
    int max_seq_len, int max_dec_len, int fuse_softmax, int early_stop, float length_penalty, int P,
    float* part, int* ids_out, float* cum_out, int* cache_ids, int* beam_offsets, int* parent_out,
    unsigned char* stop_out, int* seq_lens_out, int* step_ids_out, hipStream_t st);
PIAMD_EXPORT int piamd_argmax_rows(const void* x, long long ld, int R, int V, int dtype,
    long long* out, hipStream_t st);

// ---- viterbi.hip
PIAMD_EXPORT int piamd_viterbi_decode(const float* pot, const float* trans,
    const long long* lengths, int B, int T, int N, int bos_eos, float* scores, long long* path,
    int* hist, hipStream_t stream);

// ---- xent.hip
PIAMD_EXPORT int piamd_xent_stats(int dtype, const void* logits, const long long* labels, int rows,
    int V, long long vocab_start, int ignore_index, float* out_max, float* out_sum,
    float* out_target, hipStream_t stream);
PIAMD_EXPORT int piamd_xent_bwd(int dtype, const void* logits, const long long* labels,
    const float* lse, const float* dloss, float dloss_scalar, int rows, int V,
    long long vocab_start, int ignore_index, void* grad, hipStream_t stream);
