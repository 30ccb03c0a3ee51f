// Stand-alone driver of mx::sk_takes (csrc/kernels/skinny_args.h), the one operand check of the skinny
// decode GEMM launchers: reads one launch description per line from stdin -- `key=value` tokens,
// integers in any base strtoll takes, addresses as integers (never dereferenced), missing keys 0 --
// and prints per line `<sk_takes> <the former launcher's guard>` as 1 (taken) or 0 (refused).  The
// guards are the six `if (...) return -1;` expressions the launchers carried before the check was
// unified, transcribed verbatim: the oracle of tests/test_skinny_args.py, which builds this file plain
// and under AddressSanitizer + UBSan (the M * K product must not overflow).
#include "kernels/skinny_args.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

using namespace mx;

// ---- the former guards (M >= 1), each with its launcher's parameter names
static bool old_skinny_gemm(int64_t ldx, int64_t ldw, int64_t ldy, int M, int N, int K) {
  if (M > 32 || N % 16 || K % 512 || ldx % 8 || ldw % 8 || ldy % 4 || ldx < K || ldw < K || ldy < N) return false;
  return true;
}
static bool old_skinny_gemm_swiglu(int64_t ldx, int64_t ldw, int64_t ldy, int M, int F, int K) {
  if (M > 32 || F % 8 || K % 512 || ldx % 8 || ldw % 8 || ldy % 4 || ldx < K || ldw < K || ldy < F) return false;
  return true;
}
static bool old_skinny_norm_gemm(int64_t ldh, const uint16_t* delta, int64_t ldd, uint16_t* h_out, int64_t ldw,
                                 int64_t ldy, int M, int N, int K, int swiglu) {
  if (M > 4 || (int64_t)M * K > 32768 || N % 16 || K % 512 || ldh % 8 || ldd % 8 || ldw % 8 || ldy % 4 ||
      ldh < K || ldw < K || (delta && (ldd < K || !h_out)))
    return false;
  if (swiglu) {
    const int Fh = N / 2;
    if (Fh % 8 || ldy < Fh) return false;
  } else {
    if (ldy < N) return false;
  }
  return true;
}
static bool old_skinny_rope_gemm(int64_t ldh, int norm, const uint16_t* delta, int64_t ldd, uint16_t* h_out,
                                 int64_t ldw, int M, int K) {
  if (M > (norm ? 4 : 16) || (norm && (int64_t)M * K > 32768) || K % 512 || ldh % 8 || ldd % 8 || ldw % 8 ||
      ldh < K || ldw < K || (norm && delta && (ldd < K || !h_out)))
    return false;
  return true;
}
static bool old_skinny_merge_gemm(int nsplit, int64_t ldw, int64_t ldy, int M, int N, int K) {
  if (M > 4 || (int64_t)M * K > 32768 || N % 16 || K % 512 || ldw % 8 || ldy % 4 || ldw < K || ldy < N ||
      nsplit < 1)
    return false;
  return true;
}
static bool old_w8a16_gemm(int64_t ldx, int64_t ldy, int M, int N, int K) {
  if (M > 32 || N % 16 || K % 512 || ldx % 8 || ldy % 4 || ldx < K || ldy < N) return false;
  return true;
}

static bool old_guard(const SkLaunch& L) {
  switch (L.entry) {
    case SK_PLAIN: return old_skinny_gemm(L.X.ld, L.W.ld, L.Y.ld, L.M, L.N, L.K);
    case SK_SWIGLU: return old_skinny_gemm_swiglu(L.X.ld, L.W.ld, L.Y.ld, L.M, L.N / 2, L.K);
    case SK_NORM:
      return old_skinny_norm_gemm(L.X.ld, L.na.delta, L.na.ldd, L.na.h_out, L.W.ld, L.Y.ld, L.M, L.N, L.K, L.swiglu);
    case SK_ROPE: return old_skinny_rope_gemm(L.X.ld, L.norm, L.na.delta, L.na.ldd, L.na.h_out, L.W.ld, L.M, L.K);
    case SK_MERGE: return old_skinny_merge_gemm(L.mg.nsplit, L.W.ld, L.Y.ld, L.M, L.N, L.K);
    case SK_W8: return old_w8a16_gemm(L.X.ld, L.Y.ld, L.M, L.N, L.K);
  }
  return false;
}

static int name_index(const std::string& v, const char* const* names, int n) {
  for (int i = 0; i < n; ++i)
    if (v == names[i]) return i;
  return (int)strtol(v.c_str(), nullptr, 0);  // a number: also values outside the enum
}

int main() {
  static const char* const entries[] = {"plain", "swiglu", "norm", "rope", "merge", "w8"};
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    SkLaunch L{};
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
      if (k == "entry") L.entry = (SkEntry)name_index(v, entries, 6);
      else if (k == "x") L.X.p = p;
      else if (k == "ldx") L.X.ld = i;
      else if (k == "w") L.W.p = p;
      else if (k == "ldw") L.W.ld = i;
      else if (k == "y") L.Y.p = p;
      else if (k == "ldy") L.Y.ld = i;
      else if (k == "M") L.M = (int)i;
      else if (k == "N") L.N = (int)i;
      else if (k == "K") L.K = (int)i;
      else if (k == "swiglu") L.swiglu = (int)i;
      else if (k == "norm") L.norm = (int)i;
      else if (k == "delta") L.na.delta = (const uint16_t*)p;
      else if (k == "ldd") L.na.ldd = i;
      else if (k == "gamma") L.na.gamma = (const uint16_t*)p;
      else if (k == "h_out") L.na.h_out = (uint16_t*)p;
      else if (k == "cosb") L.rp.cosb = (const float*)p;
      else if (k == "sinb") L.rp.sinb = (const float*)p;
      else if (k == "pos") L.rp.pos = (const int32_t*)p;
      else if (k == "slots") L.rp.slots = (const int32_t*)p;
      else if (k == "q") L.rp.q = (uint16_t*)p;
      else if (k == "kc") L.rp.kc = (uint16_t*)p;
      else if (k == "vc") L.rp.vc = (uint16_t*)p;
      else if (k == "Hq") L.rp.Hq = (int)i;
      else if (k == "Hkv") L.rp.Hkv = (int)i;
      else if (k == "max_seq") L.rp.max_seq = (int)i;
      else if (k == "bt") L.rp.bt = (const int32_t*)p;
      else if (k == "maxb") L.rp.maxb = (int)i;
      else if (k == "ml") L.mg.ml = (const float*)p;
      else if (k == "po") L.mg.po = (const float*)p;
      else if (k == "nsplit") L.mg.nsplit = (int)i;
      else if (k == "scale") L.scale = (const float*)p;
      else {
        fprintf(stderr, "unknown key %s\n", k.c_str());
        return 2;
      }
    }
    printf("%d %d\n", sk_takes(L) ? 1 : 0, old_guard(L) ? 1 : 0);
  }
  return 0;
}
