// Experiment: v_mfma_i32_32x32x32_i8 as the engine of the L1 2-NN lower bound (l1k2_prune.hip).
// (1) layout: lane l supplies 16 consecutive k of A row l%32 and of B column l%32, k-half l/32; the
//     same k-to-lane map on both sides, so any map gives the exact integer GEMM.  D register v of lane
//     l is row 8*(v/4) + 4*(l/32) + v%4, column l%32.  Checked against a host GEMM on asymmetric ints.
// (2) rate: cycles per instruction back to back, 2 waves per SIMD.
// (3) the same with every second wave running a v_sad_u8 chain instead: do the two pipes overlap?
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

__global__ void layout(const int8_t *A, const int8_t *B, int *D, int K) {  // A [32][K], B [32][K] (column major B) -> D [32][32]
  const int l = threadIdx.x, r = l & 31, g = l >> 5;
  v16i c = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int k0 = 0; k0 < K; k0 += 32) {
    const v4i a = *reinterpret_cast<const v4i *>(A + r * K + k0 + 16 * g);
    const v4i b = *reinterpret_cast<const v4i *>(B + r * K + k0 + 16 * g);
    c = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c, 0, 0, 0);
  }
  for (int v = 0; v < 16; ++v) D[(8 * (v >> 2) + 4 * g + (v & 3)) * 32 + r] = c[v];
}

// mode 0: every wave MFMA; mode 1: odd waves of a workgroup run SADs instead; mode 2: only even waves work (MFMA);
// mode 3: only odd waves work (SAD)
__global__ __launch_bounds__(512) void rate(int *out, int iters, int mode) {
  const int w = threadIdx.x >> 6;
  const bool sad = (mode == 1 || mode == 3) && (w & 4);  // waves 4..7 = second wave of each SIMD
  const bool idle = (mode == 2 && (w & 4)) || (mode == 3 && !(w & 4));
  int res = 0;
  if (idle) {
  } else if (!sad) {
    v16i c0 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, c1 = c0;
    v4i a = {(int)threadIdx.x, 3, 5, 7}, b = {1, (int)threadIdx.x * 3, 2, 9};
    for (int i = 0; i < iters; ++i) {
      c0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, c0, 0, 0, 0);
      c1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(b, a, c1, 0, 0, 0);
    }
    res = c0[0] + c1[5];
  } else {
    unsigned s0 = threadIdx.x, s1 = 1, s2 = 2, s3 = 3;
    const unsigned a = threadIdx.x * 2654435761u, b = threadIdx.x * 40503u + 17;
    for (int i = 0; i < iters * 4; ++i) {  // 16 SADs per trip = 64 cycles = two MFMAs' worth
      s0 = __builtin_amdgcn_sad_u8(a, b, s0); s1 = __builtin_amdgcn_sad_u8(a, s0, s1);
      s2 = __builtin_amdgcn_sad_u8(a, b, s2); s3 = __builtin_amdgcn_sad_u8(b, s2, s3);
      s0 = __builtin_amdgcn_sad_u8(a, b, s0); s1 = __builtin_amdgcn_sad_u8(a, s0, s1);
      s2 = __builtin_amdgcn_sad_u8(a, b, s2); s3 = __builtin_amdgcn_sad_u8(b, s2, s3);
      s0 = __builtin_amdgcn_sad_u8(a, b, s0); s1 = __builtin_amdgcn_sad_u8(a, s0, s1);
      s2 = __builtin_amdgcn_sad_u8(a, b, s2); s3 = __builtin_amdgcn_sad_u8(b, s2, s3);
      s0 = __builtin_amdgcn_sad_u8(a, b, s0); s1 = __builtin_amdgcn_sad_u8(a, s0, s1);
      s2 = __builtin_amdgcn_sad_u8(a, b, s2); s3 = __builtin_amdgcn_sad_u8(b, s2, s3);
    }
    res = s0 + s1 + s2 + s3;
  }
  out[blockIdx.x * blockDim.x + threadIdx.x] = res;
}

int main() {
  const int K = 512;
  std::vector<int8_t> A(32 * K), B(32 * K);
  std::vector<int> D(32 * 32);
  srand(5);
  for (auto &v : A) v = (int8_t)(rand() % 255 - 127);
  for (auto &v : B) v = (int8_t)(rand() % 200 - 60);
  int8_t *dA, *dB; int *dD;
  hipMalloc(&dA, A.size()); hipMalloc(&dB, B.size()); hipMalloc(&dD, D.size() * 4);
  hipMemcpy(dA, A.data(), A.size(), hipMemcpyHostToDevice); hipMemcpy(dB, B.data(), B.size(), hipMemcpyHostToDevice);
  hipLaunchKernelGGL(layout, dim3(1), dim3(64), 0, 0, dA, dB, dD, K);
  hipMemcpy(D.data(), dD, D.size() * 4, hipMemcpyDeviceToHost);
  int ok = 0;
  for (int i = 0; i < 32; ++i) for (int j = 0; j < 32; ++j) {
    int c = 0; for (int k = 0; k < K; ++k) c += (int)A[i * K + k] * (int)B[j * K + k];
    ok += c == D[i * 32 + j];
  }
  printf("i32_32x32x32_i8 layout: %d/1024 match the host GEMM (D[v] = row 8*(v/4)+4*(lane/32)+v%%4, col lane%%32)\n", ok);
  int *out; hipMalloc(&out, 256 * 512 * 4);
  hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
  const int iters = 100000;
  const char *names[] = {"mfma on both waves of a SIMD", "mfma wave + sad wave per SIMD", "mfma wave alone", "sad wave alone"};
  for (int mode = 0; mode < 4; ++mode) {
    float ms = 0;
    for (int rep = 0; rep < 2; ++rep) {
      hipEventRecord(e0);
      hipLaunchKernelGGL(rate, dim3(256), dim3(512), 0, 0, out, iters, mode);  // one 8-wave workgroup per CU
      hipEventRecord(e1); hipEventSynchronize(e1);
      hipEventElapsedTime(&ms, e0, e1);
    }
    // per wave 2*iters MFMAs (or 16*iters SADs)
    printf("%-32s %.3f ms = %.1f cycles per 2 MFMA (or 16 SAD) trip of one wave at 2.4 GHz\n", names[mode], ms,
           ms * 1e-3 * 2.4e9 / iters);
  }
  return 0;
}
