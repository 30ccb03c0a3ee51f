// Stand-alone driver of mx::af_takes, mx::ab_takes and the backward's workspace / partial-head arithmetic
// (csrc/kernels/attn_args.h): reads one launch per line from stdin -- `key=value` tokens, integers in any
// base strtoll takes, addresses as integers (never dereferenced), missing keys 0 except `on` (1) and `hpw`
// (mx::ab_hpw of the line, with `on` and `forced`) -- and prints per line
// `<af_takes> <ab_takes> <ab_shape_takes> <ab_s_pad> <ab_key_blocks> <ab_work_bytes> <hpw> <ab_partial_heads>
//  <ab_ds_bytes_per_head> <ab_takes_rope>` (the arithmetic as -1 where ab_shape_takes refuses the line).
// tests/test_attn_args.py builds this file plain and under AddressSanitizer + UBSan: the products of the
// overflow rules must not overflow themselves.
#include "kernels/attn_args.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

using namespace mx;

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    AfLaunch F{};
    AbLaunch L{};
    long long on = 1, forced = 0;
    bool hpw_given = false;
    std::istringstream ss(line);
    std::string tok;
    while (ss >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) {
        fprintf(stderr, "bad token %s\n", tok.c_str());
        return 2;
      }
      const std::string k = tok.substr(0, eq), v = tok.substr(eq + 1);
      const long long i = strtoll(v.c_str(), nullptr, 0);
      void* p = reinterpret_cast<void*>((uintptr_t)strtoull(v.c_str(), nullptr, 0));
      if (k == "q") F.q = L.q = p;
      else if (k == "k") F.k = L.k = p;
      else if (k == "v") F.v = L.v = p;
      else if (k == "o") F.o = p, L.o = p;
      else if (k == "lse") F.lse = p, L.lse = p;
      else if (k == "dout") L.dout = p;
      else if (k == "delta") L.delta = p;
      else if (k == "dq") L.dq = p;
      else if (k == "dkp") L.dkp = p;
      else if (k == "dvp") L.dvp = p;
      else if (k == "work") L.work = p;
      else if (k == "dqkv") L.dqkv = p;
      else if (k == "cos") L.cos = p;
      else if (k == "sin") L.sin = p;
      else if (k == "q_bf16") F.q_bf16 = L.q_bf16 = (int)i;
      else if (k == "kv_bf16") F.kv_bf16 = L.kv_bf16 = (int)i;
      else if (k == "o_bf16") F.o_bf16 = L.o_bf16 = (int)i;
      else if (k == "lse_f32") F.lse_f32 = L.lse_f32 = (int)i;
      else if (k == "dout_bf16") L.dout_bf16 = (int)i;
      else if (k == "out_f32") L.out_f32 = (int)i;
      else if (k == "dqkv_bf16") L.dqkv_bf16 = (int)i;
      else if (k == "B") F.B = L.B = i;
      else if (k == "Hq") F.Hq = L.Hq = i;
      else if (k == "Hkv") F.Hkv = L.Hkv = i;
      else if (k == "S") F.S = L.S = i;
      else if (k == "Sk") F.Sk = L.Sk = i;
      else if (k == "D") F.D = L.D = i;
      else if (k == "ldo") F.ldo = L.ldo = i;
      else if (k == "ldq") L.ldq = i;
      else if (k == "cos_rows") L.cos_rows = i;
      else if (k == "causal") F.causal = L.causal = (int)i;
      else if (k == "dq_mode") L.dq_mode = (int)i;
      else if (k == "hpw") L.hpw = i, hpw_given = true;
      else if (k == "on") on = i;
      else if (k == "forced") forced = i;
      else {
        fprintf(stderr, "unknown key %s\n", k.c_str());
        return 2;
      }
    }
    if (!hpw_given) L.hpw = ab_hpw(L.B, L.Hq, L.Hkv, L.Sk, L.D, L.dq_mode, on != 0, forced);
    const bool shape = ab_shape_takes(L), arith = shape && !ab_empty(L);
    printf("%d %d %d %lld %lld %lld %lld %lld %lld %d\n", af_takes(F) ? 1 : 0, ab_takes(L) ? 1 : 0, shape ? 1 : 0,
           arith ? (long long)ab_s_pad(L.S) : -1, arith ? (long long)ab_key_blocks(L.Sk) : -1,
           arith ? (long long)ab_work_bytes(L) : -1, (long long)L.hpw,
           arith ? (long long)ab_partial_heads(L.B, L.Hq, L.Hkv, L.Sk, L.D, L.dq_mode, on != 0, forced) : -1,
           arith ? (long long)ab_ds_bytes_per_head(L.S, L.Sk) : -1, ab_takes_rope(L.dq_mode, L.D, L.S, L.Sk) ? 1 : 0);
  }
  return 0;
}
