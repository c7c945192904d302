// Experiment: v_mfma_scale_f32_32x32x64_f8f6f4 with FP6 (e2m3) operands as the engine of the L1 2-NN lower bound
// (l1k2_prune.hip, the FP6 form).  An e2m3 value is k/8, k in {0..15, 16..30 step 2, 32..60 step 4}, either sign, so a
// product is a multiple of 1/64 and a sum far below 2^24/64 is exact in f32 IF the instruction adds exactly.
// (1) exactness: one 64 x 64 x 640 product (2 x 2 blocks of 32 x 32, 10 k-steps of 64, scale bytes 0x7F on both sides)
//     against an int64 host GEMM, bit for bit, on random codes, on all +-7.5, and with accumulators started at minus the
//     sum (the result must be +0.0, sign bit clear) and one step of 1/64 either side of it.
//     Operand layout: lane l supplies 32 consecutive k of A row l%32 and of B column l%32, k-half l/32, as 32 six-bit
//     codes packed little-endian into 6 dwords; the same k-to-lane map on both sides, so any map gives the exact GEMM.
// (2) rate: cycles per instruction back to back, two waves and one wave per SIMD, beside v_mfma_i32_32x32x32_i8.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef float v16f __attribute__((ext_vector_type(16)));

constexpr int kK = 640, kSteps = kK / 64, kRowBytes = kK * 6 / 8;  // 480 bytes per row: k-step s, lane half g at 48 s + 24 g

__device__ __forceinline__ v8i load6(const uint8_t *p) {
  const uint32_t *q = reinterpret_cast<const uint32_t *>(p);
  v8i v = {(int)q[0], (int)q[1], (int)q[2], (int)q[3], (int)q[4], (int)q[5], 0, 0};
  return v;
}

// A [64][480 B], B [64][480 B] (rows of B are columns of the product), C0 and D [64][64] floats
__global__ void gemm(const uint8_t *A, const uint8_t *B, const float *C0, float *D) {
  const int l = threadIdx.x, r = l & 31, g = l >> 5;
  const int scale = 0x7F7F7F7F;
  for (int h = 0; h < 2; ++h)
    for (int b = 0; b < 2; ++b) {
      v16f c;
      for (int v = 0; v < 16; ++v) c[v] = C0[(32 * h + 8 * (v >> 2) + 4 * g + (v & 3)) * 64 + 32 * b + r];
      for (int s = 0; s < kSteps; ++s) {
        const v8i a = load6(A + (32 * h + r) * kRowBytes + 48 * s + 24 * g);
        const v8i bb = load6(B + (32 * b + r) * kRowBytes + 48 * s + 24 * g);
        c = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, bb, c, 2, 2, 0, scale, 0, scale);
      }
      for (int v = 0; v < 16; ++v) D[(32 * h + 8 * (v >> 2) + 4 * g + (v & 3)) * 64 + 32 * b + r] = c[v];
    }
}

// kind 0: fp6 scaled MFMA, kind 1: int8 MFMA; both_waves 0: waves 4..7 (the second wave of each SIMD) idle
__global__ __launch_bounds__(512) void rate(int *out, int iters, int kind, int both_waves) {
  const int w = threadIdx.x >> 6;
  int res = 0;
  if (both_waves || !(w & 4)) {
    if (kind == 0) {
      v16f c0 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, c1 = c0;
      const int t = threadIdx.x & 7;  // small codes: the sums stay finite
      v8i a = {t, 3, 5, 7, 1, 2, 0, 0}, b = {1, t * 3, 2, 9, 4, 6, 0, 0};
      const int scale = 0x7F7F7F7F;
      for (int i = 0; i < iters; ++i) {
        c0 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c0, 2, 2, 0, scale, 0, scale);
        c1 = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(b, a, c1, 2, 2, 0, scale, 0, scale);
      }
      res = (int)(c0[0] + c1[5]);
    } else {
      v16i c0 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, c1 = c0;
      v4i a = {(int)threadIdx.x, 3, 5, 7}, b = {1, (int)threadIdx.x * 3, 2, 9};
      for (int i = 0; i < iters; ++i) {
        c0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(b, a, c1, 0, 0, 0);
      }
      res = c0[0] + c1[5];
    }
  }
  out[blockIdx.x * blockDim.x + threadIdx.x] = res;
}

#define CHECK(e)                                                                  \
  do {                                                                            \
    hipError_t err_ = (e);                                                        \
    if (err_ != hipSuccess) {                                                     \
      fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(err_));                   \
      return 2;                                                                   \
    }                                                                             \
  } while (0)

static int k_of(int code) {  // the integer k of a 6-bit e2m3 code, value k/8
  const int c = code & 31, k = c < 16 ? c : c < 24 ? 2 * (c - 8) : 4 * (c - 16);
  return code & 32 ? -k : k;
}
static void pack(const std::vector<uint8_t> &codes, std::vector<uint8_t> &rows) {  // [64][640] codes -> [64][480] bytes
  rows.assign(64 * kRowBytes, 0);
  for (int i = 0; i < 64; ++i)
    for (int k = 0; k < kK; ++k) {
      const int bit = 6 * k;
      const uint32_t v = codes[i * kK + k] & 63u;
      rows[i * kRowBytes + bit / 8] |= (uint8_t)(v << (bit % 8));
      if (bit % 8 > 2) rows[i * kRowBytes + bit / 8 + 1] |= (uint8_t)(v >> (8 - bit % 8));
    }
}

int main() {
  uint8_t *dA, *dB;
  float *dC, *dD;
  CHECK(hipMalloc(&dA, 64 * kRowBytes));
  CHECK(hipMalloc(&dB, 64 * kRowBytes));
  CHECK(hipMalloc(&dC, 64 * 64 * 4));
  CHECK(hipMalloc(&dD, 64 * 64 * 4));
  srand(5);
  int bad_total = 0;
  // fill 0: random codes; 1: all +-7.5, the sign by row and column; 2: random magnitudes, all positive (large sums)
  // start 0: accumulators at 0; 1: at -sum (the result is +0.0); 2: at -sum - 1/64; 3: at -sum + 1/64
  const char *fills[] = {"random codes", "all +-7.5", "random positive codes"};
  const char *starts[] = {"C = 0", "C = -sum", "C = -sum - 1/64", "C = -sum + 1/64"};
  for (int fill = 0; fill < 3; ++fill)
    for (int start = 0; start < 4; ++start) {
      std::vector<uint8_t> ca(64 * kK), cb(64 * kK), ra, rb;
      for (int i = 0; i < 64; ++i)
        for (int k = 0; k < kK; ++k) {
          if (fill == 0) {
            ca[i * kK + k] = rand() & 63;
            cb[i * kK + k] = rand() & 63;
          } else if (fill == 1) {
            ca[i * kK + k] = 31 | ((i * 7 + k) % 3 == 0 ? 32 : 0);
            cb[i * kK + k] = 31 | ((i * 5 + k) % 5 < 2 ? 32 : 0);
          } else {
            ca[i * kK + k] = rand() & 31;
            cb[i * kK + k] = rand() & 31;
          }
        }
      pack(ca, ra);
      pack(cb, rb);
      std::vector<long long> S(64 * 64);
      std::vector<float> C0(64 * 64), want(64 * 64), D(64 * 64);
      long long smax = 0;
      for (int i = 0; i < 64; ++i)
        for (int j = 0; j < 64; ++j) {
          long long s = 0;
          for (int k = 0; k < kK; ++k) s += (long long)k_of(ca[i * kK + k]) * k_of(cb[j * kK + k]);
          S[i * 64 + j] = s;
          smax = std::max(smax, s < 0 ? -s : s);
          const long long c0 = start == 0 ? 0 : start == 1 ? -s : start == 2 ? -s - 1 : -s + 1;
          C0[i * 64 + j] = (float)c0 / 64.0f;           // |c0| < 2^24: exact
          want[i * 64 + j] = (float)(c0 + s) / 64.0f;   // 0 is +0.0f
        }
      CHECK(hipMemcpy(dA, ra.data(), ra.size(), hipMemcpyHostToDevice));
      CHECK(hipMemcpy(dB, rb.data(), rb.size(), hipMemcpyHostToDevice));
      CHECK(hipMemcpy(dC, C0.data(), C0.size() * 4, hipMemcpyHostToDevice));
      hipLaunchKernelGGL(gemm, dim3(1), dim3(64), 0, 0, dA, dB, dC, dD);
      CHECK(hipDeviceSynchronize());
      CHECK(hipMemcpy(D.data(), dD, D.size() * 4, hipMemcpyDeviceToHost));
      int bad = 0;
      float worst = 0;
      for (int e = 0; e < 64 * 64; ++e) {
        if (memcmp(&D[e], &want[e], 4) != 0) {
          if (!bad) printf("    first mismatch at (%d, %d): got %.9g (0x%08x), want %.9g\n", e / 64, e % 64, D[e], *(uint32_t *)&D[e], want[e]);
          ++bad;
          worst = std::max(worst, std::abs(D[e] - want[e]));
        }
      }
      printf("f8f6f4 e2m3 64x64x640, %-22s %-16s max |sum| %8lld/64: %d/4096 differ bit for bit (max error %.6g)\n", fills[fill],
             starts[start], smax, bad, worst);
      bad_total += bad;
    }
  printf("exactness: %s\n", bad_total ? "NOT EXACT" : "exact on every entry of every case");

  int *out;
  CHECK(hipMalloc(&out, 256 * 512 * 4));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  const int iters = 100000;
  const char *kinds[] = {"v_mfma_scale_f32_32x32x64_f8f6f4 (fp6)", "v_mfma_i32_32x32x32_i8"};
  for (int kind = 0; kind < 2; ++kind)
    for (int both = 1; both >= 0; --both) {
      float ms = 0;
      for (int rep = 0; rep < 2; ++rep) {
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(rate, dim3(256), dim3(512), 0, 0, out, iters, kind, both);  // one 8-wave workgroup per CU
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        CHECK(hipEventElapsedTime(&ms, e0, e1));
      }
      // per wave 2 * iters MFMAs
      printf("%-40s %s: %.3f ms = %.1f cycles per 2 MFMAs of one wave at 2.4 GHz\n", kinds[kind],
             both ? "both waves of a SIMD" : "one wave per SIMD   ", ms, ms * 1e-3 * 2.4e9 / iters);
    }
  return bad_total ? 1 : 0;
}
