// Host-side description of a verify-attention launch (decode.hip verify_attn_kernel: decode attention
// for up to n consecutive query rows per sequence) and THE check that says whether the launch is
// taken.  Plain C++: no HIP, no torch -- the launcher, the torch bindings and the stand-alone test
// (tests/native/test_verify_args.cpp) include this one file.  The launcher calls vf_takes before it
// enqueues anything, so a refusal (-1) always means "nothing launched, nothing written".
// nq and lens live on the device (the step is graphed), so the check cannot read them: the kernel
// clamps nq[b] into [0, n] and lens[b] + nq[b] into the slot's capacity.
#pragma once
#include <stdint.h>

namespace mx {

constexpr int VF_SPLIT = 256;    // keys per workgroup (decode.hip kSplit)
constexpr int VF_MAX_COLS = 32;  // (row, head) columns of one (sequence, KV head): two MFMA blocks of 16

struct VfLaunch {
  const void* q;           // [B * n, Hq, D] bf16: row b * n + j is query row j of sequence b
  const void* k_pool;      // [rows, Hkv, max_seq, D] bf16 or e4m3 codes (u8); paged: [blocks, Hkv, block, D]
  const void* v_pool;
  const float* k_scale;    // kv8: [rows, Hkv, max_seq] f32 scale pools (nullptr with bf16 pools)
  const float* v_scale;
  const int32_t* lens;     // device [B]: L_b, keys of the slot before the new rows
  const int32_t* nq;       // device [B]: new rows of sequence b, at positions L_b .. L_b + nq[b] - 1
  const int32_t* slots;    // device [B] cache slot (nullptr: b)
  const int32_t* bt;       // device block table [slots, maxb] (nullptr: contiguous caches)
  float* part_ml;          // [B * n, Hq, nsplit, 2]
  float* part_o;           // [B * n, Hq, nsplit, D]
  void* out;               // [B * n, Hq * D] bf16
  int q_bf16, out_bf16;    // element types of q and out
  int kv_bf16, kv_u8;      // element type of both pools: exactly one is set
  int64_t B, n, Hq, Hkv, D;
  int64_t rows, max_seq, maxb;  // pool rows; the pools' sequence dimension (paged: the block size)
  int64_t nsplit;
};

// Whether the launch is taken (B >= 1: the launcher returns 0 for B <= 0 before it asks).
inline bool vf_takes(const VfLaunch& L) {
  constexpr int64_t I32 = 0x7fffffff;
  if (!L.q || !L.k_pool || !L.v_pool || !L.lens || !L.nq || !L.part_ml || !L.part_o || !L.out) return false;
  // bf16 q and out; bf16 pools without scales, or u8 code pools with both f32 scale pools
  if (!L.q_bf16 || !L.out_bf16) return false;
  if (!!L.kv_bf16 == !!L.kv_u8) return false;
  if (L.kv_u8 ? (!L.k_scale || !L.v_scale) : (L.k_scale || L.v_scale)) return false;
  // the D = 128 MFMA tiling
  if (L.D != 128) return false;
  // whole GQA groups; the n rows of a group are at most 32 columns
  if (L.Hq <= 0 || L.Hkv <= 0 || L.Hq % L.Hkv) return false;
  if (L.n < 1 || L.n > VF_MAX_COLS / (L.Hq / L.Hkv)) return false;
  if (L.B <= 0 || L.nsplit <= 0 || L.rows <= 0 || L.max_seq <= 0) return false;
  // paged: a 256-key split lies inside one block
  if (L.bt && (L.maxb <= 0 || L.max_seq % VF_SPLIT)) return false;
  // grid (nsplit, Hkv, B)
  if (L.Hkv > 65535 || L.B > 65535) return false;
  // 32-bit values of the kernel: key positions (split * 256, the slot's capacity), the row b * n + j,
  // the combine grid B * n * Hq (as divisions: the products themselves must not overflow)
  if (L.nsplit > I32 / VF_SPLIT || L.max_seq > I32) return false;
  if (L.bt && L.maxb > I32 / L.max_seq) return false;
  if (L.B > I32 / L.n || L.B * L.n > I32 / L.Hq) return false;
  return true;
}

}  // namespace mx
