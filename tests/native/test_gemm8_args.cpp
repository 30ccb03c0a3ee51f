// Stand-alone driver of mx::g8_takes (csrc/kernels/gemm8_args.h), the one operand check of the gemm8
// launchers: reads one launch description per line from stdin -- `key=value` tokens, integers in any
// base strtoll takes, addresses as integers (never dereferenced), missing keys 0 -- and prints 1
// (taken) or 0 (refused) per line.  tests/test_gemm8_args.py feeds it the rule grid, built plain and
// under AddressSanitizer + UBSan (the span arithmetic must not overflow).
#include "kernels/gemm8_args.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

static int name_index(const std::string& v, const char* const* names, int n) {
  for (int i = 0; i < n; ++i)
    if (v == names[i]) return i;
  return (int)strtol(v.c_str(), nullptr, 0);  // a number: also values outside the enum
}

int main() {
  static const char* const entries[] = {"plain", "sq", "epi", "tail", "rope_tail"};
  static const char* const epis[] = {"none", "rope", "swiglu", "swiglu_bwd"};
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    mx::G8Launch L{};
    L.C.kc = 1;
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
      const void* p = reinterpret_cast<const void*>((uintptr_t)strtoull(v.c_str(), nullptr, 0));
      if (k == "entry") L.entry = (mx::G8Entry)name_index(v, entries, 5);
      else if (k == "epi") L.epi = name_index(v, epis, 4);
      else if (k == "a") L.A.p = p;
      else if (k == "lda") L.A.ld = i;
      else if (k == "a_kc") L.A.kc = (int)i;
      else if (k == "b") L.B.p = p;
      else if (k == "ldb") L.B.ld = i;
      else if (k == "b_kc") L.B.kc = (int)i;
      else if (k == "c") L.C.p = p;
      else if (k == "ldc") L.C.ld = i;
      else if (k == "out_f32") L.out_f32 = (int)i;
      else if (k == "M") L.M = (int)i;
      else if (k == "N") L.N = (int)i;
      else if (k == "K") L.K = (int)i;
      else if (k == "beta") L.beta = (float)strtod(v.c_str(), nullptr);
      else if (k == "rows") L.rows = (int)i;
      else if (k == "at") L.at = (int)i;
      else if (k == "ws") L.ws = p;
      else if (k == "ph") L.ph = (int)i;
      else if (k == "sq") L.ep.sq = (float*)p;
      else if (k == "q") L.ep.q = (uint16_t*)p;
      else if (k == "k") L.ep.k = (uint16_t*)p;
      else if (k == "v") L.ep.v = (uint16_t*)p;
      else if (k == "cosb") L.ep.cosb = (const float*)p;
      else if (k == "sinb") L.ep.sinb = (const float*)p;
      else if (k == "S") L.ep.S = (int)i;
      else if (k == "Hq") L.ep.Hq = (int)i;
      else if (k == "Hkv") L.ep.Hkv = (int)i;
      else if (k == "m") L.ep.m = (uint16_t*)p;
      else if (k == "ldm") L.ep.ldm = i;
      else if (k == "gu") L.ep.gu = (const uint16_t*)p;
      else if (k == "ldg") L.ep.ldg = i;
      else {
        fprintf(stderr, "unknown key %s\n", k.c_str());
        return 2;
      }
    }
    puts(mx::g8_takes(L) ? "1" : "0");
  }
  return 0;
}
