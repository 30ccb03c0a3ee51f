// C launch API of the mxllm gfx950 kernels (csrc/kernels/*.hip), grouped by the file that defines
// each entry point.  Every kernel file includes this header, so each definition is compiled against
// its declaration (C linkage: a drifted parameter list is a compile error, not scrambled arguments);
// default arguments live here only.  Torch-free.
// All functions return 0 on success, a hipError_t (>0) or -1 on bad arguments.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "kernels/attn_args.h"
#include "kernels/gemm8_args.h"
#include "kernels/prefill_paged_args.h"
#include "kernels/skinny_args.h"
#include "kernels/verify_args.h"
#include "kernels/w4_args.h"

extern "C" {
// attn_bwd.hip (operand rules: mx::ab_takes, kernels/attn_args.h)
// sets L.hpw (mx::ab_hpw under MXLLM_ATTN_BWD8 / _HPW) and returns the dK / dV partial heads per batch row
int mx_attn_bwd_partial_heads(mx::AbLaunch& L);
int mx_attn_bwd(const mx::AbLaunch& L, float scale, hipStream_t stream);

// attn_fwd.hip (operand rules: mx::af_takes, kernels/attn_args.h)
int mx_attn_fwd(const mx::AfLaunch& L, float scale, hipStream_t stream);

// cross_entropy.hip
int mx_ce_fwd_bwd(uint16_t* logits, const int64_t* labels, float* losses, float* inv_n, float* loss_out, int64_t T,
                  int V, int64_t ignore, hipStream_t stream);
int mx_ce_inv_count(const int64_t* labels, int64_t T, int V, int64_t ignore, float* inv_n, hipStream_t stream);
int mx_ce_chunk(uint16_t* logits, const int64_t* labels, float* losses, const float* inv_n, int64_t T, int V,
                int64_t ignore, hipStream_t stream);
int mx_ce_chunk_f32(const float* logits, uint16_t* dl, const int64_t* labels, float* losses, const float* inv_n,
                    int64_t T, int V, int64_t ignore, hipStream_t stream);

// decode.hip
int mx_rope_append(const uint16_t* qkv, const float* cosb, const float* sinb, const int32_t* pos, const int32_t* slots,
                   uint16_t* q, uint16_t* kc, uint16_t* vc, int B, int Hq, int Hkv, int D, int max_seq,
                   const int32_t* bt, int maxb, hipStream_t stream);
int mx_decode_attn(const uint16_t* q, const uint16_t* kc, const uint16_t* vc, const int32_t* lens, int len_off,
                   const int32_t* slots, float* part_ml, float* part_o, uint16_t* out, int B, int Hq, int Hkv, int D,
                   int max_seq, int nsplit, float scale, const int32_t* bt, int maxb, unsigned int* cnt,
                   hipStream_t stream);
int mx_kv8_quant_rows(const uint16_t* x, int64_t ldx, uint8_t* q, float* s, int64_t R, hipStream_t stream);
int mx_rope_append_kv8(const uint16_t* qkv, const float* cosb, const float* sinb, const int32_t* pos,
                       const int32_t* slots, uint16_t* q, uint8_t* kq, float* ks, uint8_t* vq, float* vs, int B, int Hq,
                       int Hkv, int max_seq, const int32_t* bt, int maxb, hipStream_t stream);
int mx_decode_attn_kv8(const uint16_t* q, const uint8_t* kq, const float* ks, const uint8_t* vq, const float* vs,
                       const int32_t* lens, int len_off, const int32_t* slots, float* part_ml, float* part_o,
                       uint16_t* out, int B, int Hq, int Hkv, int max_seq, int nsplit, float scale, const int32_t* bt,
                       int maxb, hipStream_t stream);
// verify_attn / verify_attn_kv8 (operand rules: mx::vf_takes, kernels/verify_args.h)
int mx_verify_attn(const mx::VfLaunch& L, float scale, hipStream_t stream);
int64_t mx_sample_ws_floats(int B);
int mx_sample(const void* logits, int is_bf16, int64_t* out, int B, int V, float temperature, uint32_t seed,
              uint32_t step, float* ws, hipStream_t stream);
int mx_sample_temp_rows(const void* logits, int is_bf16, int64_t* out, int B, int V, const float* temps,
                        const int64_t* seeds, const int32_t* steps, float* ws, hipStream_t stream);

// elementwise.hip
int mx_swiglu_fwd(const uint16_t* gu, uint16_t* m, int64_t T, int F, int64_t ldm, hipStream_t stream);
int mx_swiglu_bwd(const uint16_t* dm, const uint16_t* gu, uint16_t* dgu, int64_t T, int F, int64_t ldg,
                  hipStream_t stream, uint16_t* m = nullptr);
int mx_adamw(float* p, void* g, int grad_bf16, float* m, float* v, uint16_t* lowp, int16_t* lo, int64_t n,
             float lr, float b1, float b2, float eps, float wd, float bc1, float bc2, const float* scale_t,
             float scale_f, int zero_grad, hipStream_t stream);
int mx_split_master(const float* x, uint16_t* hi, int16_t* lo, int64_t n, hipStream_t stream);
int mx_join_master(const uint16_t* hi, const int16_t* lo, float* x, int64_t n, hipStream_t stream);
int mx_embedding_fwd(const int64_t* ids, const uint16_t* w, uint16_t* out, int64_t T, int H, int64_t V,
                     hipStream_t stream);
int mx_embedding_bwd_sorted(const uint16_t* dy, const int64_t* sid, const int64_t* perm, int64_t T, int H,
                            int64_t V, void* out, int out_f32, float* ws, hipStream_t stream);
int mx_embedding_bwd(const int64_t* ids, const uint16_t* dy, float* dw, int64_t T, int H, int64_t V,
                     hipStream_t stream);

// fp8_gemm.hip
int mx_w8a16_gemm(const uint16_t* x, int64_t ldx, const uint8_t* q, const float* scale, uint16_t* y, int64_t ldy,
                  int M, int N, int K, hipStream_t stream);
int mx_quant_rows_e4m3(const uint16_t* x, int64_t ldx, uint8_t* q, float* s, int64_t M, int K, hipStream_t stream);
int mx_w8_dequant(const uint8_t* q, const float* scale, uint16_t* w, int64_t N, int K, hipStream_t stream);

// mxfp4_gemm.hip (operand rules of the GEMM: mx::w4_takes, kernels/w4_args.h)
int mx_w4a16_gemm(const mx::W4Launch& L, hipStream_t stream);
int mx_w4_dequant(const uint8_t* codes, const uint8_t* scales, uint16_t* w, int64_t N, int64_t K, hipStream_t stream);

// gemm8.hip (operand rules of every entry point: mx::g8_takes, kernels/gemm8_args.h)
int mx_gemm8(const uint16_t* A, int64_t lda, int a_kc, const uint16_t* B, int64_t ldb, int b_kc, void* C,
             int64_t ldc, int out_f32, int M, int N, int K, float beta, const float* alpha_t, float alpha_f,
             int ph, hipStream_t stream);
int mx_gemm8_epi(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, uint16_t* C, int64_t ldc, int M,
                 int N, int K, mx::G8EpiMode mode, mx::G8Epi ep, hipStream_t stream);
int mx_gemm8_sq(const uint16_t* A, int64_t lda, int a_kc, const uint16_t* B, int64_t ldb, int b_kc, uint16_t* C,
                int64_t ldc, int M, int N, int K, const float* alpha_t, float alpha_f, float* sq, hipStream_t stream);
int mx_gemm8_tail(const uint16_t* A, int64_t lda, int a_kc, const uint16_t* B, int64_t ldb, int b_kc, uint16_t* C,
                  int64_t ldc, int M, int N, int K, int rows, int at, float* ws, int ph, hipStream_t stream,
                  float* sq = nullptr);
int mx_gemm8_rope_tail(const uint16_t* A, int64_t lda, const uint16_t* B, int64_t ldb, int M, int N, int K, int at,
                       float* ws, mx::G8Epi ep, hipStream_t stream);
int mx_gemm8_stamps(unsigned long long* host);

// logits_proc.hip
int mx_logits_adjust_rows(const void* logits, int is_bf16, float* out, int B, int V, const int32_t* state,
                          const int32_t* slots, int n_slots, const float* presence, const float* frequency,
                          const float* repetition, const float* bias, hipStream_t stream);
int mx_token_state_update(int32_t* state, const int32_t* slots, const int64_t* ids, int B, int V, int n_slots,
                          hipStream_t stream);
int64_t mx_logprob_ws_bytes(int B, int V);
int mx_logprob_rows(const void* logits, int is_bf16, const int64_t* ids, const int32_t* n_top, float* chosen_lp,
                    int32_t* top_ids, float* top_lp, int B, int V, void* ws, hipStream_t stream);

// lora.hip
int64_t mx_swiglu_lora_ws(int T, int F, int nrb);
int mx_swiglu_lora(int bwd, const uint16_t* gu, const uint16_t* dm, uint16_t* out, int64_t ldo, const uint16_t* V,
                   int64_t ldv, int nrb, int pad, float alpha, float* ws, int T, int F, hipStream_t stream);
int64_t mx_lora_xwt_ws(int M, int K, int rows);
int64_t mx_lora_xtg_ws(int ntiles, int T);
int mx_lora_xwt(const uint16_t* X, int64_t ldx, const uint16_t* V, int64_t ldv, int Vrows, uint16_t* out, int64_t ldo,
                float* ws, int M, int K, float alpha, int rows, hipStream_t stream);
int mx_lora_xtg(const int64_t* desc, int np, int T, float alpha, int accumulate, float* ws, hipStream_t stream);

// lora_serve.hip
int mx_lora_serve_ksplits(int K);
int mx_lora_gather_shrink(const uint16_t* x, int64_t ldx, const int32_t* ids, const uint16_t* a_tab, float* part,
                          int M, int K, int R, int n_adapters, hipStream_t stream);
int mx_lora_gather_expand_add(uint16_t* y, int64_t ldy, const float* part, const int32_t* ids, const uint16_t* b_tab,
                              const float* s_tab, int M, int N, int KS, int r_max, const int* splits, int n_splits,
                              int n_adapters, hipStream_t stream);

// misc.hip
int mx_copy2d_batched(const int64_t* desc, int n, int64_t total_blocks, hipStream_t stream);
int mx_segmented_mean_i32(const int32_t* codes, const int64_t* offs, float* out, int nseg,
                          hipStream_t stream);
int mx_sqnorm(const void* x, int bf16, int64_t n, float* out, float* work, hipStream_t stream);
int mx_transpose16(const void* in, void* out, int64_t R, int64_t C, int64_t ld_in, int64_t ld_out,
                   const float* scale, hipStream_t stream);
int mx_prefetch(const void* p, int64_t bytes, int wgs, hipStream_t stream);

// peer_coll.hip (called from runtime/peer_comm.cpp)
size_t mx_peer_staging_bytes(int world, int wgs, int slot_bytes);
size_t mx_peer_staging_bytes2(int world, int wgs, int slot_bytes, int64_t light_cap);
int mx_peer_collective_light(int mode, int dtype, int wire, char* const* lbases, const void* in, void* out,
                             int64_t n, int64_t m, int rank, int world, int wgs, int64_t light_cap,
                             uint32_t* epoch, int* err, long long timeout_ticks, hipStream_t stream);
int mx_peer_collective(int mode, int dtype, char* const* bases, const void* in, void* out, int64_t n,
                       int64_t m, int rank, int world, int wgs, int slot_bytes, uint32_t* epochs, int* err,
                       long long timeout_ticks, hipStream_t stream);

// prefill_paged.hip (operand rules: mx::pp_takes, kernels/prefill_paged_args.h)
int mx_prefill_attn_paged(const mx::PpLaunch& L, float scale, hipStream_t stream);

// rmsnorm.hip
int mx_rmsnorm_fwd(const uint16_t* x, const uint16_t* res, const uint16_t* w, uint16_t* y,
                   uint16_t* h_out, float* rstd, int T, int H, int ldy, float eps, hipStream_t stream);
int mx_rmsnorm_bwd(const uint16_t* dy, const uint16_t* x, const uint16_t* w, const float* rstd,
                   const uint16_t* dres, uint16_t* dx, float* dwp, int T, int H, int ldr, int ldx, int rpb,
                   hipStream_t stream);
int mx_colsum_f32(const float* p, float* out, int nblk, int H, hipStream_t stream);

// rope.hip
int mx_rope_split(const uint16_t* qkv, const float* cosb, const float* sinb, const int32_t* positions, uint16_t* q,
                  uint16_t* k, uint16_t* v, int B, int S, int Hq, int Hkv, int D, hipStream_t stream);
int mx_rope_merge_bwd(const float* dq, const float* dkp, const float* dvp, const float* cosb, const float* sinb,
                      uint16_t* dqkv, int B, int S, int Hq, int Hkv, int kv_heads_in, int D, int64_t ldq,
                      hipStream_t stream, int head0);

// sampling.hip
int mx_sample_rows(const void* logits, int is_bf16, int64_t* out, int B, int V, const float* temps,
                   const float* top_ps, const int32_t* top_ks, const int64_t* seeds, const int32_t* steps,
                   hipStream_t stream);

int mx_spec_accept(const int64_t* drawn, const int64_t* tokens, const int32_t* nq, int32_t* out, int B, int n,
                   hipStream_t stream);

// skinny_gemm.hip (operand rules of every entry: mx::sk_takes, kernels/skinny_args.h; the same
// rules hold for mx_w8a16_gemm above)
int mx_skinny(const mx::SkLaunch& L, hipStream_t stream);

// xgmi.hip (called from runtime/xgmi_comm.cpp)
int mx_xgmi_allreduce(uint32_t* const* flags, float* const* data, const float* in, float* out, int n,
                      int rank, int world, uint32_t epoch, int max_elems, int op, int* err,
                      long long timeout_ticks, hipStream_t stream);
int mx_xgmi_allreduce_bf16(uint32_t* const* flags, uint16_t* const* data, const uint16_t* in,
                           uint16_t* out, int n, int rank, int world, int max_elems, uint32_t* epochs,
                           int* err, long long timeout_ticks, hipStream_t stream);
}
