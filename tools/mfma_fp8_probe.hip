// One v_mfma_scale_f32_16x16x128_f8f6f4 (e4m3 x e4m3, scales 1, C = 0) per
// wave against float64: the worst |d - exact| / sum_k |a_k b_k| over many
// random products, in units of 2^-23. Times nothing. The figures behind
// MFMA_COEFF of tests/test_gpu_linear_fp8_a8.py (profiles/linear_fp8_a8.md).
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -o mfma_fp8_probe \
//       tools/mfma_fp8_probe.hip && ./mfma_fp8_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) int i32x8;

__global__ __launch_bounds__(64) void probe(const unsigned char* A,
                                            const unsigned char* B, float* D) {
  const int lane = threadIdx.x;
  const size_t blk = (size_t)blockIdx.x * 16 * 128;
  const size_t off = blk + (lane & 15) * 128 + (lane >> 4) * 32;
  const i32x8 a = *(const i32x8*)(A + off);
  const i32x8 b = *(const i32x8*)(B + off);
  f32x4 c = {0.f, 0.f, 0.f, 0.f};
  c = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a, b, c, 0, 0, 0,
                                                       0x7F7F7F7F, 0,
                                                       0x7F7F7F7F);
  for (int j = 0; j < 4; ++j)
    D[(size_t)blockIdx.x * 256 + ((lane >> 4) * 4 + j) * 16 + (lane & 15)] = c[j];
}

static double dec(unsigned char b) {
  const int e = (b >> 3) & 15, m = b & 7;
  const double v = e == 0 ? m * std::ldexp(1.0, -9)
                          : (1.0 + m / 8.0) * std::ldexp(1.0, e - 7);
  return (b & 0x80) ? -v : v;
}

static unsigned char enc_nearest(double v) {  // nearest code, ties unimportant
  int best = 0;
  double bd = 1e300;
  for (int c = 0; c < 256; ++c) {
    if ((c & 0x7F) == 0x7F) continue;
    const double d = std::fabs(dec((unsigned char)c) - v);
    if (d < bd) { bd = d; best = c; }
  }
  return (unsigned char)best;
}

#define CK(e) do { hipError_t r_ = (e); if (r_ != hipSuccess) { \
  std::printf("HIP error %s at %d\n", hipGetErrorString(r_), __LINE__); return 2; } } while (0)

int main() {
  const int NB = 2048;
  const size_t n = (size_t)NB * 16 * 128;
  std::mt19937_64 rng(7);
  for (int dist = 0; dist < 3; ++dist) {
    // 0: uniform codes, K = 128; 1: gaussian rows scaled to absmax 448,
    // K = 128; 2: as 1 with k >= 64 zero (the zero-filled tail)
    std::vector<unsigned char> A(n), B(n);
    std::normal_distribution<double> g(0.0, 1.0);
    for (auto* M : {&A, &B})
      for (size_t r = 0; r < n / 128; ++r) {
        if (dist == 0) {
          for (int k = 0; k < 128; ++k) {
            unsigned char c;
            do c = (unsigned char)(rng() & 0xFF); while ((c & 0x7F) == 0x7F);
            (*M)[r * 128 + k] = c;
          }
        } else {
          double v[128], amax = 0;
          const int kk = dist == 2 ? 64 : 128;
          for (int k = 0; k < 128; ++k) {
            v[k] = k < kk ? g(rng) : 0.0;
            amax = std::fmax(amax, std::fabs(v[k]));
          }
          for (int k = 0; k < 128; ++k)
            (*M)[r * 128 + k] = enc_nearest(v[k] / amax * 448.0);
        }
      }
    unsigned char *dA, *dB;
    float* dD;
    CK(hipMalloc(&dA, n)); CK(hipMalloc(&dB, n));
    CK(hipMalloc(&dD, (size_t)NB * 256 * 4));
    CK(hipMemcpy(dA, A.data(), n, hipMemcpyHostToDevice));
    CK(hipMemcpy(dB, B.data(), n, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(probe, dim3(NB), dim3(64), 0, 0, dA, dB, dD);
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    std::vector<float> D((size_t)NB * 256);
    CK(hipMemcpy(D.data(), dD, D.size() * 4, hipMemcpyDeviceToHost));
    double worst = 0, worst_rel_max = 0;
    size_t exact_n = 0;
    for (int b = 0; b < NB; ++b)
      for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j) {
          double s = 0, S = 0, pmax = 0;
          for (int k = 0; k < 128; ++k) {
            const double p = dec(A[((size_t)b * 16 + i) * 128 + k]) *
                             dec(B[((size_t)b * 16 + j) * 128 + k]);
            s += p; S += std::fabs(p); pmax = std::fmax(pmax, std::fabs(p));
          }
          const double err = std::fabs((double)D[(size_t)b * 256 + i * 16 + j] - s);
          if (err == 0) ++exact_n;
          if (S > 0) worst = std::fmax(worst, err / S);
          if (pmax > 0) worst_rel_max = std::fmax(worst_rel_max, err / pmax);
        }
    std::printf("MFMA_PROBE|dist=%d|elements=%zu|exact=%zu|worst err/sum|ab| = "
                "%.3f * 2^-23|worst err/max|ab| = %.3f * 2^-23\n", dist,
                (size_t)NB * 256, exact_n, worst * 8388608.0,
                worst_rel_max * 8388608.0);
    CK(hipFree(dA)); CK(hipFree(dB)); CK(hipFree(dD));
  }
  return 0;
}
