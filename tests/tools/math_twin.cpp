// The host twin of gym_kmanip_amd/csrc/kmanip_math.hpp (tests/test_math_cpu.py): the header UNMODIFIED, compiled
// for the host behind a shim directory whose hip/hip_runtime.h is empty.  The two hardware estimates are replaced by seeds with a
// 24-bit mantissa (frexp, round to float, ldexp): not the hardware's values, so the twin holds everything BUT the estimates -- the
// polynomials, the reductions, the selects, the Newton steps -- to the device's bars.
//   g++ -O2 -ffp-contract=off -I<shim> -I<csrc> math_twin.cpp -o math_twin
//   math_twin <sincos|atan2|sqrt|rcp> <rows> <in.f64> <out.f64>       raw little-endian doubles, row-major
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define __device__
#define __forceinline__ inline
static inline double km_twin_seed(double v) {
  if (!std::isfinite(v) || v == 0) return v;
  int e;
  const double m = std::frexp(v, &e);
  return std::ldexp((double)(float)m, e);
}
#define __builtin_amdgcn_rcp(x) km_twin_seed(1.0 / (x))
#define __builtin_amdgcn_rsq(x) km_twin_seed(1.0 / std::sqrt(x))
#include "kmanip_math.hpp"

int main(int argc, char** argv) {
  if (argc != 5) { std::fprintf(stderr, "usage: math_twin fn rows in out\n"); return 2; }
  const char* fn = argv[1];
  const size_t n = (size_t)std::atol(argv[2]);
  const int ic = !std::strcmp(fn, "atan2") ? 2 : 1, oc = !std::strcmp(fn, "sincos") ? 2 : 1;
  std::vector<double> in(n * ic), out(n * oc);
  FILE* f = std::fopen(argv[3], "rb");
  if (!f || std::fread(in.data(), sizeof(double), in.size(), f) != in.size()) { std::fprintf(stderr, "math_twin: cannot read %s\n", argv[3]); return 2; }
  std::fclose(f);
  for (size_t i = 0; i < n; i++) {
    if (!std::strcmp(fn, "sincos")) km_sincos(in[i], &out[2 * i], &out[2 * i + 1]);
    else if (!std::strcmp(fn, "atan2")) out[i] = km_atan2(in[2 * i], in[2 * i + 1]);
    else if (!std::strcmp(fn, "sqrt")) out[i] = km_sqrt(in[i]);
    else if (!std::strcmp(fn, "rcp")) out[i] = km_rcp(in[i]);
    else { std::fprintf(stderr, "math_twin: no function %s\n", fn); return 2; }
  }
  f = std::fopen(argv[4], "wb");
  if (!f || std::fwrite(out.data(), sizeof(double), out.size(), f) != out.size()) { std::fprintf(stderr, "math_twin: cannot write %s\n", argv[4]); return 2; }
  std::fclose(f);
  return 0;
}
