// sift.hip -- vlfeat-exact SIFT (include/spectavi_amd.h, sift_filter) on gfx950.
//
// One image runs as a chain of kernels on one stream; every count lives on the device, so the host
// never waits between octaves.  Per octave:
//   upsample / downsample -> 5 Gaussian smoothings (vertical then horizontal pass, taps in p-ascending
//   order) -> extremum count per DoG row -> scan -> extremum write (ballot order = x order) -> refine
//   (one lane per candidate) -> scan + scatter of the survivors -> gradients -> orientation (one wave
//   per keypoint) -> scan of the angle counts -> descriptor (one wave per keypoint, its angles in turn).
// Every float sum keeps vlfeat's order: a histogram bin is owned by one lane, which adds the window's
// pixels in raster order; the pixels' terms are computed 64 at a time, one per lane, through LDS.
// The DoG is never stored: D[s] = L[s+1] - L[s] is recomputed where it is read (same float result).
// Many images run as one such chain (sift_batch_run): the same bodies, the image as one more grid dimension.
#include "common.h"
#include "host_io.h"

#include <math.h>

#include <cmath>

namespace spv {
namespace {

constexpr int kMaxTaps = 32;  // 2W+1 with W = ceil(4 sigma) <= 13 for the default settings
constexpr int kScanThreads = 1024, kScanItems = 8;
constexpr int kPersistBlocks = 2048;
constexpr int kKeyBlocks = 8192;  // one-wave blocks of the keypoint kernels: about 8 waves per SIMD
constexpr float kTwoPiF = (float)(2 * M_PI);
constexpr float kFltEps = 1.19209290e-07f;

struct Taps {
  int W;
  float t[kMaxTaps];
};

enum { C_NCAND = 0, C_KP_LO = 2, C_KP_HI = 3, C_NROW = 4, C_COUNT = 8 };  // device counters

// ---- vlfeat's fast approximations (vl/mathop.h), bit for bit ------------------------------
__device__ __forceinline__ float fast_resqrt_f(float x) {
  const float xhalf = 0.5f * x;
  float y = __int_as_float(0x5f3759df - (__float_as_int(x) >> 1));
  y = y * (1.5f - xhalf * y * y);
  y = y * (1.5f - xhalf * y * y);
  return y;
}
__device__ __forceinline__ float fast_sqrt_f(float x) { return ((double)x < 1e-8) ? 0.f : x * fast_resqrt_f(x); }
__device__ __forceinline__ float fast_atan2_f(float y, float x) {
  const float ay = fabsf(y) + kFltEps;
  float r, a;
  if (x >= 0) {
    r = (x - ay) / (x + ay);
    a = (float)(M_PI / 4);
  } else {
    r = (x + ay) / (ay - x);
    a = (float)(3 * M_PI / 4);
  }
  a += (0.1821f * r * r - 0.9675f) * r;
  return (y < 0) ? -a : a;
}
__device__ __forceinline__ float mod2pi_f(float x) {
  while (x > kTwoPiF) x -= kTwoPiF;
  while (x < 0.f) x += kTwoPiF;
  return x;
}
// vlfeat's fast_expn table, expn_tab[k] = exp(-k * 25/256), k = 0..256, as the C library's exp gives
// it (written out in hexadecimal; tests/test_sift_oracle.py checks every entry against the host's exp).
// Constant data: no per-call upload, nothing for a captured stream to copy.
__constant__ double kExpn[257] = {
    0x1.0000000000000p+0, 0x1.d05d24612c2afp-1, 0x1.a528e2e1d9f0ap-1, 0x1.7df9ab76b20fdp-1,
    0x1.5a6fc061433c8p-1, 0x1.3a344c42322f0p-1, 0x1.1cf88def26e0ap-1, 0x1.0275180612d31p-1,
    0x1.d4d244cf4ea9ep-2, 0x1.a933d7dd220fcp-2, 0x1.81a455c174b70p-2, 0x1.5dc31577a457ep-2,
    0x1.3d386c3dec4f1p-2, 0x1.1fb4d761f3916p-2, 0x1.04f039fb35bfdp-2, 0x1.d952597135e09p-3,
    0x1.ad48bc25771c7p-3, 0x1.855802b8b74a7p-3, 0x1.611e969df99c8p-3, 0x1.4043f5a4b1409p-3,
    0x1.2277d9b6eed30p-3, 0x1.077174b6623bep-3, 0x1.dddd7d31ec28cp-4, 0x1.b167a824c0132p-4,
    0x1.8914c880e4177p-4, 0x1.648257e94a907p-4, 0x1.4356faad37142p-4, 0x1.2541a572fde00p-4,
    0x1.09f8d73309544p-4, 0x1.e273cb3ea1e33p-5, 0x1.b590b480e26f2p-5, 0x1.8cdabd74cef83p-5,
    0x1.67ee6d9ff847cp-5, 0x1.46718dbaf5fd5p-5, 0x1.28124b439e06ep-5, 0x1.0c8670916d4adp-5,
    0x1.e7155f0750059p-6, 0x1.b9c3fa1c5598cp-6, 0x1.90a9f8263b0acp-6, 0x1.6b62ec3a36a9ep-6,
    0x1.4993c15e964fbp-6, 0x1.2ae9dbff486bap-6, 0x1.0f1a5016fc0f8p-6, 0x1.ebc2543f5c374p-7,
    0x1.be019216b7bdap-7, 0x1.94828f5e61af9p-7, 0x1.6edfe86286e1cp-7, 0x1.4cbda8565f8a9p-7,
    0x1.2dc868a5d6beap-7, 0x1.11b4852eaa984p-7, 0x1.f07ac6de3e81ep-8, 0x1.c24995cd64169p-8,
    0x1.98649a1e7ad48p-8, 0x1.726576f632fa2p-8, 0x1.4fef558ea8751p-8, 0x1.30ae0260e8ea3p-8,
    0x1.14551f6951195p-8, 0x1.f53ed32028990p-9, 0x1.c69c1edc0a9ebp-9, 0x1.9c502fa0468eap-9,
    0x1.75f3ad05caa9dp-9, 0x1.5328dc22484e3p-9, 0x1.339aba844bbb1p-9, 0x1.16fc2e7e08200p-9,
    0x1.fa0e9586aebc7p-10, 0x1.caf9471d49400p-10, 0x1.a04567569805cp-10, 0x1.798a9fd5a152dp-10,
    0x1.566a4f5b0912cp-10, 0x1.368ea28e60847p-10, 0x1.19a9c24a8692ap-10, 0x1.feea2ad9723a3p-11,
    0x1.cf6128ab46776p-11, 0x1.a44458ede1b5fp-11, 0x1.7d2a64de4d371p-11, 0x1.59b3c2b21adc4p-11,
    0x1.3989cc2885c2dp-11, 0x1.1c5dead380970p-11, 0x1.01e8d81366c98p-11, 0x1.d3d3dde04d757p-12,
    0x1.a84d1c4cc3094p-12, 0x1.80d311cd27e54p-12, 0x1.5d0549d0885b3p-12, 0x1.3c8c492780c05p-12,
    0x1.1f18b84507626p-12, 0x1.0462a16241230p-12, 0x1.d85181576bbeap-13, 0x1.ac5fc994974d9p-13,
    0x1.8484bc84cfe21p-13, 0x1.605ef88fac6fbp-13, 0x1.3f962b8be83bfp-13, 0x1.21da3af2e9f4dp-13,
    0x1.06e280283423ap-13, 0x1.dcda2ded104edp-14, 0x1.b07c79220609fp-14, 0x1.883f7b1dab8f7p-14,
    0x1.63c0e2f9a8e2ep-14, 0x1.42a785829017cp-14, 0x1.24a2835916c22p-14, 0x1.096883588f934p-14,
    0x1.e16dfebfac43bp-15, 0x1.b4a3438d94b63p-15, 0x1.8c0363e66d558p-15, 0x1.672b1d49de448p-15,
    0x1.45c06964f60f0p-15, 0x1.2771a21bfe4b3p-15, 0x1.0bf4ba0b60739p-15, 0x1.e60d0f305512ap-16,
    0x1.b8d441ac39d8fp-16, 0x1.8fd08d649910ep-16, 0x1.6a9dbbed64ee7p-16, 0x1.48e0e9b9af77ap-16,
    0x1.2a47a808f6a91p-16, 0x1.0e87337dcb492p-16, 0x1.eab77ae3684c4p-17, 0x1.bd0f8c8ff18f3p-17,
    0x1.93a70e550ac81p-17, 0x1.6e18d38387323p-17, 0x1.4c091934d811bp-17, 0x1.2d24a616a00cep-17,
    0x1.111fff1267413p-17, 0x1.ef6d5dc130f34p-18, 0x1.c1553d885380ap-18, 0x1.9786fdac7eac7p-18,
    0x1.719c78de3cb24p-18, 0x1.4f390ab881e69p-18, 0x1.3008ad654a370p-18, 0x1.13bf2c519a381p-18,
    0x1.f42ed3f68e690p-19, 0x1.c5a56e232a448p-19, 0x1.9b7072981a695p-19, 0x1.7528c102a6eadp-19,
    0x1.5270d155263bbp-19, 0x1.32f3cf3f5ae74p-19, 0x1.1664cae9f5a18p-19, 0x1.f8fbf9f59cf4cp-20,
    0x1.ca00382d0c3afp-20, 0x1.9f63847df7c46p-20, 0x1.78bdc1298eec5p-20, 0x1.55b0804a179a8p-20,
    0x1.35e61d19b548ap-20, 0x1.1910eab094556p-20, 0x1.fdd4ec765fe86p-21, 0x1.ce65b5b1f5dd3p-21,
    0x1.a3604afdb0929p-21, 0x1.7c5b8ebfe44aep-21, 0x1.58f82b05f4f0ap-21, 0x1.38dfa894225bep-21,
    0x1.1bc39ba17942dp-21, 0x1.015ce43bb6b40p-21, 0x1.d2d600fde589ap-22, 0x1.a766ddf0ec058p-22,
    0x1.80023f673d463p-22, 0x1.5c47e5271dcafp-22, 0x1.3be08379ba61ep-22, 0x1.1e7ceddfef0c4p-22,
    0x1.03d5559f4debap-22, 0x1.d751349d78ce7p-23, 0x1.ab77556bed539p-23, 0x1.83b1e8f6582bcp-23,
    0x1.5f9fc27c27ae6p-23, 0x1.3ee8bfc14f499p-23, 0x1.213cf1b6e88e3p-23, 0x1.0653d92cd8784p-23,
    0x1.dbd76b5e8b36ap-24, 0x1.af91c9be23bebp-24, 0x1.876aa1799df72p-24, 0x1.62ffd70454914p-24,
    0x1.41f86f8dd8235p-24, 0x1.2403b79962533p-24, 0x1.08d87dcf8945ap-24, 0x1.e068c050d69d9p-25,
    0x1.b3b65372bbfd3p-25, 0x1.8b2c7f33a633bp-25, 0x1.666836f00a773p-25, 0x1.450fa52edd9c4p-25,
    0x1.26d15022c4f78p-25, 0x1.0b6352973c89fp-25, 0x1.e5054ec6950c7p-26, 0x1.b7e50b513307ep-26,
    0x1.8ef7989dbc21dp-26, 0x1.69d8f6a14c339p-26, 0x1.482e7320e7842p-26, 0x1.29a5cc17487e7p-26,
    0x1.0df466b8d1dd4p-26, 0x1.e9ad325524257p-27, 0x1.bc1e0a5dea510p-27, 0x1.92cc04686523dp-27,
    0x1.6d522aac33545p-27, 0x1.4b54ec0deb60ap-27, 0x1.2c813c64589bap-27, 0x1.108bc98e872e7p-27,
    0x1.ee6086d5aa206p-28, 0x1.c06169dabd671p-28, 0x1.96a9d97be874bp-28, 0x1.70d3e7d76b38ap-28,
    0x1.4e8322cdbc100p-28, 0x1.2f63b220f9f30p-28, 0x1.13298a9854973p-28, 0x1.f31f6865bc5d0p-29,
    0x1.c4af434799080p-29, 0x1.9a912ef8d82cep-29, 0x1.745e431cad55bp-29, 0x1.51b92a667a7e3p-29,
    0x1.324d3e8e3051ap-29, 0x1.15cdb97c49126p-29, 0x1.f7e9f368078e9p-30, 0x1.c907b06313a6ep-30,
    0x1.9e821c389b973p-30, 0x1.77f151a93ead8p-30, 0x1.54f7160d076f4p-30, 0x1.353df31765e12p-30,
    0x1.18786606e8158p-30, 0x1.fcc04484f9849p-31, 0x1.cd6acb2b07690p-31, 0x1.a27cb8cdfada6p-31,
    0x1.7b8d28de6e794p-31, 0x1.583cf9257660dp-31, 0x1.3835e152d359bp-31, 0x1.1b29a02b88108p-31,
    0x1.00d13c55b64a6p-31, 0x1.d1d8addd2d9d0p-32, 0x1.a6811c85abf93p-32, 0x1.7f31de52160b7p-32,
    0x1.5b8ae74381863p-32, 0x1.3b351b01e9334p-32, 0x1.1de17804b1d61p-32, 0x1.03485688aa553p-32,
    0x1.d65172f7bbb04p-33, 0x1.aa8f5f66e12d7p-33, 0x1.82df87cf19ebfp-33, 0x1.5ee0f42afee18p-33,
    0x1.3e3bb211b9d9bp-33, 0x1.209ffdd480eddp-33, 0x1.05c57f9a36ff7p-33, 0x1.dad5353a01a5dp-34,
    0x1.aea799b3d8a06p-34, 0x1.86963b55ec320p-34, 0x1.623f33d0567cap-34, 0x1.4149b89b64e5cp-34,
    0x1.2365420504d3cp-34, 0x1.0848c66d76bfcp-34, 0x1.df640fa50a132p-35, 0x1.b2c9e3ea6d850p-35,
    0x1.8a560f1d101d6p-35, 0x1.65a5ba58f9c47p-35, 0x1.445f40e4835dbp-35, 0x1.26315528a3260p-35,
    0x1.0ad23a0a19728p-35, 0x1.e3fe1d7c3ba50p-36, 0x1.b6f656c4aa962p-36, 0x1.8e1f19919ef44p-36,
    0x1.69149c1bdc096p-36, 0x1.477c5d5f94ff9p-36, 0x1.290447fa7ac4cp-36, 0x1.0d61e99cbe402p-36,
    0x1.e8a37a45fc32ep-37,
};

__device__ __forceinline__ double fast_expn(const double *tab, double x) {
  if (x > 25.0) return 0.0;
  x *= 256 / 25.0;
  const int i = (int)floor(x);
  const double r = x - i;
  const double a = tab[i], b = tab[min(i + 1, 256)];
  return a + r * (b - a);
}

// ---- scale space --------------------------------------------------------------------------
// out (2h x 2w) from in (h x w): x pass, then y pass, as copy_and_upsample_rows twice.
__device__ __forceinline__ float up_x(const float *in, int w, int r, int X) {
  const int i = X >> 1;
  if (!(X & 1)) return in[(size_t)r * w + i];
  if (i < w - 1) return (in[(size_t)r * w + i] + in[(size_t)r * w + i + 1]) * 0.5f;
  return in[(size_t)r * w + w - 1];
}
// The kernels' bodies take their place in the grid as arguments: the single-image kernels and the batch
// kernels (one more grid dimension: the image) run the same code, hence write the same bits.
__device__ __forceinline__ void upsample_body(const float *__restrict__ in, int w, int h, float *__restrict__ out, int X, int Y) {
  if (X >= 2 * w) return;
  const int i = Y >> 1;
  float v;
  if (!(Y & 1)) v = up_x(in, w, i, X);
  else if (i < h - 1) v = (up_x(in, w, i, X) + up_x(in, w, i + 1, X)) * 0.5f;
  else v = up_x(in, w, h - 1, X);
  out[(size_t)Y * 2 * w + X] = v;
}
__global__ __launch_bounds__(256) void sift_upsample_kernel(const float *__restrict__ in, int w, int h, float *__restrict__ out) {
  upsample_body(in, w, h, out, blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y);
}

__device__ __forceinline__ void downsample_body(const float *__restrict__ in, int win, float *__restrict__ out, int w, int x, int y) {
  if (x >= w) return;
  out[(size_t)y * w + x] = in[(size_t)(2 * y) * win + 2 * x];
}
__global__ __launch_bounds__(256) void sift_downsample_kernel(const float *__restrict__ in, int win, float *__restrict__ out, int w) {
  downsample_body(in, win, out, w, blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y);
}

// VERT: out[y][x] = sum_j in[clamp(y - W + j)][x] * t[2W - j]; else the same along x.
template <bool VERT>
__device__ __forceinline__ void smooth_body(const float *__restrict__ in, float *__restrict__ out, int w, int h, const Taps &tp, int x, int y) {
  if (x >= w) return;
  const int W = tp.W;
  float acc = 0.f;
  if (VERT) {
    for (int j = 0; j <= 2 * W; ++j) {
      const int p = min(max(y - W + j, 0), h - 1);
      acc += in[(size_t)p * w + x] * tp.t[2 * W - j];
    }
  } else {
    const float *row = in + (size_t)y * w;
    for (int j = 0; j <= 2 * W; ++j) {
      const int p = min(max(x - W + j, 0), w - 1);
      acc += row[p] * tp.t[2 * W - j];
    }
  }
  out[(size_t)y * w + x] = acc;
}
template <bool VERT>
__global__ __launch_bounds__(256) void sift_smooth_kernel(const float *__restrict__ in, float *__restrict__ out, int w, int h, Taps tp) {
  smooth_body<VERT>(in, out, w, h, tp, blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y);
}

// ---- extrema --------------------------------------------------------------------------------
struct Octave {
  const float *L;  // 6 levels, level index = s + 1, each h*w
  size_t plane;    // h*w
  int w, h;
  __device__ __forceinline__ float D(int di, int y, int x) const {  // di = s + 1 in 0..4
    const size_t i = (size_t)y * w + x;
    return L[(di + 1) * plane + i] - L[di * plane + i];
  }
};

__device__ __forceinline__ bool is_extremum(const Octave &oc, int di, int y, int x) {
  const float v = oc.D(di, y, x);
  bool gt = v >= 0.f, lt = v <= 0.f;
  for (int ds = -1; ds <= 1; ++ds)
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        if (ds == 0 && dy == 0 && dx == 0) continue;
        const float n = oc.D(di + ds, y + dy, x + dx);
        gt = gt && v > n;
        lt = lt && v < n;
      }
  return gt || lt;
}

// One wave per DoG row (s in 0..2, y in 1..h-2).  WRITE = false: rowcnt[r] = extrema in the row;
// WRITE = true: the row's extrema, packed x | y << 15 | s << 30, from offset rowoff[r], x ascending.
template <bool WRITE>
__device__ __forceinline__ void extrema_body(const Octave &oc, int *__restrict__ rowcnt, const int *__restrict__ rowoff,
                                             uint32_t *__restrict__ cand, int r) {
  const int lane = threadIdx.x & 63;
  const int rows = oc.h - 2;
  if (r >= 3 * rows) return;
  const int s = r / rows, y = 1 + r % rows;
  int n = WRITE ? rowoff[r] : 0;
  for (int x0 = 1; x0 <= oc.w - 2; x0 += 64) {
    const int x = x0 + lane;
    const bool hit = x <= oc.w - 2 && is_extremum(oc, s + 1, y, x);
    const uint64_t m = __ballot(hit);
    if (WRITE && hit) {
      const int below = __popcll(m & ((1ull << lane) - 1));
      cand[n + below] = (uint32_t)x | ((uint32_t)y << 15) | ((uint32_t)s << 30);
    }
    n += __popcll(m);
  }
  if (!WRITE && lane == 0) rowcnt[r] = n;
}
template <bool WRITE>
__global__ __launch_bounds__(256) void sift_extrema_kernel(Octave oc, int *__restrict__ rowcnt, const int *__restrict__ rowoff,
                                    uint32_t *__restrict__ cand) {
  extrema_body<WRITE>(oc, rowcnt, rowoff, cand, blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
}

// ---- scan ------------------------------------------------------------------------------------
// One block: out[i] = base + sum(in[lo..i)) over i in [lo, hi).  [lo, hi) is range_in[0..1] or
// [0, n); n is min(*n_dev, n) when n_dev is given.  base = *counter (0 without one).  Writes the
// total to *total_out, {base, base + total} to range_out and base + total to *counter.
__device__ __forceinline__ void scan_body(const int *__restrict__ in, int n, const int *__restrict__ n_dev,
                                          const int *__restrict__ range_in, int *out, int *counter, int *total_out,
                                          int *range_out) {
  __shared__ int part[kScanThreads];
  __shared__ int carry_s;
  int lo = 0, hi = n;
  if (range_in) {
    lo = range_in[0];
    hi = range_in[1];
  } else if (n_dev) {
    hi = min(*n_dev, n);
  }
  const int base = counter ? *counter : 0;
  const int t = threadIdx.x;
  if (t == 0) carry_s = base;
  __syncthreads();
  for (int c0 = lo; c0 < hi; c0 += kScanThreads * kScanItems) {
    int v[kScanItems], sum = 0;
    for (int k = 0; k < kScanItems; ++k) {
      const int i = c0 + t * kScanItems + k;
      v[k] = i < hi ? in[i] : 0;
      sum += v[k];
    }
    part[t] = sum;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {
      const int add = t >= d ? part[t - d] : 0;
      __syncthreads();
      part[t] += add;
      __syncthreads();
    }
    int run = carry_s + part[t] - sum;
    for (int k = 0; k < kScanItems; ++k) {
      const int i = c0 + t * kScanItems + k;
      if (i < hi) out[i] = run;
      run += v[k];
    }
    __syncthreads();
    if (t == kScanThreads - 1) carry_s += part[t];
    __syncthreads();
  }
  if (t == 0) {
    const int total = carry_s - base;
    if (total_out) *total_out = total;
    if (range_out) {
      range_out[0] = base;
      range_out[1] = base + total;
    }
    if (counter) *counter = base + total;
  }
}
__global__ __launch_bounds__(kScanThreads) void sift_scan_kernel(const int *__restrict__ in, int n,
                                                                 const int *__restrict__ n_dev,
                                                                 const int *__restrict__ range_in, int *out,
                                                                 int *counter, int *total_out, int *range_out) {
  scan_body(in, n, n_dev, range_in, out, counter, total_out, range_out);
}

// ---- refinement ------------------------------------------------------------------------------
struct KeyRec {
  float x, y, sigma;
  int s;
};

// lanes first, first + stride, ... of the image's share of the grid
__device__ __forceinline__ void refine_body(const Octave &oc, int o, double sigma0, const uint32_t *__restrict__ cand,
                                            const int *__restrict__ ncand, int *__restrict__ flag, KeyRec *__restrict__ rec,
                                            int first, int stride) {
  const int n = *ncand;
  const int w = oc.w, h = oc.h;
  for (int i = first; i < n; i += stride) {
    const uint32_t c = cand[i];
    int x = c & 0x7fff, y = (c >> 15) & 0x7fff;
    const int s = c >> 30, di = s + 1;
    double Dx = 0, Dy = 0, Ds = 0, Dxx = 0, Dyy = 0, Dxy = 0, b[3] = {0, 0, 0};
    double c0 = 0;
    int dx = 0, dy = 0;
    for (int iter = 0; iter < 5; ++iter) {
      x += dx;
      y += dy;
#define AT(ix, iy, is) oc.D(di + (is), y + (iy), x + (ix))
      c0 = (double)AT(0, 0, 0);
      Dx = 0.5 * (double)(AT(1, 0, 0) - AT(-1, 0, 0));
      Dy = 0.5 * (double)(AT(0, 1, 0) - AT(0, -1, 0));
      Ds = 0.5 * (double)(AT(0, 0, 1) - AT(0, 0, -1));
      Dxx = (double)(AT(1, 0, 0) + AT(-1, 0, 0)) - 2.0 * c0;
      Dyy = (double)(AT(0, 1, 0) + AT(0, -1, 0)) - 2.0 * c0;
      const double Dss = (double)(AT(0, 0, 1) + AT(0, 0, -1)) - 2.0 * c0;
      Dxy = 0.25 * (double)(AT(1, 1, 0) + AT(-1, -1, 0) - AT(-1, 1, 0) - AT(1, -1, 0));
      const double Dxs = 0.25 * (double)(AT(1, 0, 1) + AT(-1, 0, -1) - AT(-1, 0, 1) - AT(1, 0, -1));
      const double Dys = 0.25 * (double)(AT(0, 1, 1) + AT(0, -1, -1) - AT(0, -1, 1) - AT(0, 1, -1));
#undef AT
      double A[3][3] = {{Dxx, Dxy, Dxs}, {Dxy, Dyy, Dys}, {Dxs, Dys, Dss}};
      b[0] = -Dx;
      b[1] = -Dy;
      b[2] = -Ds;
      for (int j = 0; j < 3; ++j) {
        double maxa = 0, maxabsa = 0;
        int maxi = -1;
        for (int ii = j; ii < 3; ++ii) {
          const double a = A[ii][j], absa = fabs(a);
          if (absa > maxabsa) {
            maxa = a;
            maxabsa = absa;
            maxi = ii;
          }
        }
        if (maxabsa < (double)1e-10f) {
          b[0] = b[1] = b[2] = 0;
          break;
        }
        const int ip = maxi;
        for (int jj = j; jj < 3; ++jj) {
          const double tmp = A[ip][jj];
          A[ip][jj] = A[j][jj];
          A[j][jj] = tmp;
          A[j][jj] /= maxa;
        }
        const double tmp = b[j];
        b[j] = b[ip];
        b[ip] = tmp;
        b[j] /= maxa;
        for (int ii = j + 1; ii < 3; ++ii) {
          const double xx = A[ii][j];
          for (int jj = j; jj < 3; ++jj) A[ii][jj] -= xx * A[j][jj];
          b[ii] -= xx * b[j];
        }
      }
      for (int ii = 2; ii > 0; --ii) {
        const double xx = b[ii];
        for (int k = ii - 1; k >= 0; --k) b[k] -= xx * A[k][ii];
      }
      dx = ((b[0] > 0.6 && x < w - 2) ? 1 : 0) + ((b[0] < -0.6 && x > 1) ? -1 : 0);
      dy = ((b[1] > 0.6 && y < h - 2) ? 1 : 0) + ((b[1] < -0.6 && y > 1) ? -1 : 0);
      if (dx == 0 && dy == 0) break;
    }
    const double val = c0 + 0.5 * (Dx * b[0] + Dy * b[1] + Ds * b[2]);
    const double score = (Dxx + Dyy) * (Dxx + Dyy) / (Dxx * Dyy - Dxy * Dxy);
    const double xn = x + b[0], yn = y + b[1], sn = s + b[2];
    const bool good = fabs(val) > 0 && score < 12.1 && score >= 0 && fabs(b[0]) < 1.5 && fabs(b[1]) < 1.5 &&
                      fabs(b[2]) < 1.5 && xn >= 0 && xn <= w - 1 && yn >= 0 && yn <= h - 1 && sn >= -1 &&
                      sn <= 4;
    flag[i] = good ? 1 : 0;
    if (good) {
      const double xper = ldexp(1.0, o);
      rec[i] = KeyRec{(float)(xn * xper), (float)(yn * xper), (float)(sigma0 * pow(2.0, sn / 3) * xper), s};
    }
  }
}
__global__ __launch_bounds__(256) void sift_refine_kernel(Octave oc, int o, double sigma0, const uint32_t *__restrict__ cand, const int *__restrict__ ncand,
                                   int *__restrict__ flag, KeyRec *__restrict__ rec) {
  refine_body(oc, o, sigma0, cand, ncand, flag, rec, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

__device__ __forceinline__ void scatter_body(const int *__restrict__ ncand, const int *__restrict__ flag,
                                             const int *__restrict__ off, const KeyRec *__restrict__ rec,
                                             KeyRec *__restrict__ kp, int first, int stride) {
  const int n = *ncand;
  for (int i = first; i < n; i += stride)
    if (flag[i]) kp[off[i]] = rec[i];
}
__global__ __launch_bounds__(256) void sift_scatter_kernel(const int *__restrict__ ncand, const int *__restrict__ flag,
                                    const int *__restrict__ off, const KeyRec *__restrict__ rec,
                                    KeyRec *__restrict__ kp) {
  scatter_body(ncand, flag, off, rec, kp, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

// ---- gradients -------------------------------------------------------------------------------
// grad[(s * plane + i) * 2 + {0, 1}] = (mod, angle) of level s = 0..2 (level index s + 1).
__device__ __forceinline__ void gradient_body(const Octave &oc, float *__restrict__ grad, int x, int y, int s) {
  const int w = oc.w, h = oc.h;
  if (x >= w) return;
  const float *src = oc.L + (size_t)(s + 1) * oc.plane;
  const size_t i = (size_t)y * w + x;
  float gx, gy;
  if (x == 0) gx = src[i + 1] - src[i];
  else if (x == w - 1) gx = src[i] - src[i - 1];
  else gx = 0.5f * (src[i + 1] - src[i - 1]);
  if (y == 0) gy = src[i + w] - src[i];
  else if (y == h - 1) gy = src[i] - src[i - w];
  else gy = 0.5f * (src[i + w] - src[i - w]);
  float *g = grad + ((size_t)s * oc.plane + i) * 2;
  g[0] = fast_sqrt_f(gx * gx + gy * gy);
  g[1] = mod2pi_f((float)((double)fast_atan2_f(gy, gx) + 2 * M_PI));
}
__global__ __launch_bounds__(256) void sift_gradient_kernel(Octave oc, float *__restrict__ grad) {
  gradient_body(oc, grad, blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y, blockIdx.z);
}

// ---- orientation ------------------------------------------------------------------------------
// One 64-lane block per keypoint.  The window's pixels are taken 64 at a time in raster order, one
// per lane, into LDS; lane b < 36 then adds their terms for bin b in order (a pixel's two bins
// differ, so each bin sees the pixels in raster order, as in vlfeat).
constexpr int kSkip = -1000;  // no contribution (outside the circular window)

// blocks block, block + nblocks, ... of the image's share of the grid
__device__ __forceinline__ void orientation_body(int o, int w, int h, size_t plane, const float *__restrict__ grad,
                                                 const KeyRec *__restrict__ kp, const int *__restrict__ range,
                                                 double *__restrict__ angles, int *__restrict__ nang, int block,
                                                 int nblocks) {
  __shared__ int sb[64];
  __shared__ double sv0[64], sv1[64];
  __shared__ double hist[36];
  const int lane = threadIdx.x;
  const int lo = range[0], hi = range[1];
  const double xper = ldexp(1.0, o);
  for (int k = lo + block; k < hi; k += nblocks) {
    const KeyRec key = kp[k];
    const double x = key.x / xper, y = key.y / xper, sigma = key.sigma / xper;
    const int xi = (int)(x + 0.5), yi = (int)(y + 0.5);
    const double sigmaw = 1.5 * sigma;
    const int W = max((int)floor(3.0 * sigmaw), 1);
    const int ys0 = max(-W, -yi), ys1 = min(W, h - 1 - yi);
    const int xs0 = max(-W, -xi), xs1 = min(W, w - 1 - xi);
    const int nx = xs1 - xs0 + 1, npx = (ys1 - ys0 + 1) * nx;
    const float *g = grad + (size_t)key.s * plane * 2;
    const int b0 = (lane + 35) % 36, b1 = lane;  // pixel bins b for which this lane's bin is b + 36 or b + 1
    double acc = 0.0;
    for (int p0 = 0; p0 < npx; p0 += 64) {
      const int p = p0 + lane;
      int bin = kSkip;
      double v0 = 0, v1 = 0;
      if (p < npx) {
        const int ys = ys0 + p / nx, xs = xs0 + p % nx;
        const double dx = (double)(xi + xs) - x, dy = (double)(yi + ys) - y;
        const double r2 = dx * dx + dy * dy;
        if (r2 < W * W + 0.6) {
          const double wgt = fast_expn(kExpn, r2 / (2 * sigmaw * sigmaw));
          const float *gp = g + ((size_t)(yi + ys) * w + (xi + xs)) * 2;
          const double mod = gp[0], ang = gp[1];
          const double fbin = 36 * ang / (2 * M_PI);
          const int b = (int)floor(fbin - 0.5);
          const double rb = fbin - b - 0.5;
          bin = (b + 36) % 36;
          v0 = (1 - rb) * mod * wgt;
          v1 = rb * mod * wgt;
        }
      }
      // only the pixels inside the circle go to LDS, packed in lane (= raster) order
      const uint64_t live = __ballot(bin != kSkip);
      __syncthreads();
      if (bin != kSkip) {
        const int slot = __popcll(live & ((1ull << lane) - 1));
        sb[slot] = bin;
        sv0[slot] = v0;
        sv1[slot] = v1;
      }
      __syncthreads();
      if (lane < 36) {
        const int m = __popcll(live);
        for (int q = 0; q < m; ++q) {
          const int b = sb[q];
          if (b == b1) acc += sv0[q];       // hist[(b + 36) % 36] += (1 - rb) mod wgt
          else if (b == b0) acc += sv1[q];  // hist[(b + 1) % 36] += rb mod wgt
        }
      }
    }
    __syncthreads();
    if (lane < 36) hist[lane] = acc;
    __syncthreads();
    if (lane == 0) {  // smoothing and peaks in LDS: one lane, in vlfeat's order
      for (int it = 0; it < 6; ++it) {
        double prev = hist[35];
        const double first = hist[0];
        int i;
        for (i = 0; i < 35; ++i) {
          const double nh = (prev + hist[i] + hist[i + 1]) / 3.0;
          prev = hist[i];
          hist[i] = nh;
        }
        hist[i] = (prev + hist[i] + first) / 3.0;
      }
      double maxh = 0;
      for (int i = 0; i < 36; ++i) maxh = fmax(maxh, hist[i]);
      int na = 0;
      for (int i = 0; i < 36 && na < 4; ++i) {
        const double h0 = hist[i], hm = hist[(i + 35) % 36], hp = hist[(i + 1) % 36];
        if (h0 > 0.8 * maxh && h0 > hm && h0 > hp) {
          const double di = -0.5 * (hp - hm) / (hp + hm - 2 * h0);
          angles[(size_t)k * 4 + na++] = 2 * M_PI * (i + di + 0.5) / 36;
        }
      }
      nang[k] = na;
    }
  }
}
__global__ __launch_bounds__(64) void sift_orientation_kernel(int o, int w, int h, size_t plane,
                                                              const float *__restrict__ grad,
                                                              const KeyRec *__restrict__ kp,
                                                              const int *__restrict__ range,
                                                              double *__restrict__ angles, int *__restrict__ nang) {
  orientation_body(o, w, h, plane, grad, kp, range, angles, nang, blockIdx.x, gridDim.x);
}

// ---- descriptor --------------------------------------------------------------------------------
// One 64-lane block per keypoint, its angles in turn; lane l owns bins l and l + 64.  Pixel terms
// are computed 64 at a time into LDS; each lane then walks them in raster order and adds, for each of
// its bins that the pixel reaches, ((win mod) |1-dbx-rbx|) |1-dby-rby| |1-dbt-rbt| as vlfeat does.
__device__ __forceinline__ float bin_weight(int B, float wm, float rbx, float rby, float rbt, int bx, int by, int bt) {
  const int BY = B >> 5, BX = (B >> 3) & 3, T = B & 7;
  const int dbx = BX - 2 - bx, dby = BY - 2 - by;
  if (dbx < 0 || dbx > 1 || dby < 0 || dby > 1) return -1.f;
  int dbt;
  if (T == bt % 8) dbt = 0;
  else if (T == (bt + 1) % 8) dbt = 1;
  else return -1.f;
  return wm * fabsf((float)(1 - dbx) - rbx) * fabsf((float)(1 - dby) - rby) * fabsf((float)(1 - dbt) - rbt);
}

__device__ __forceinline__ float block_norm(float *sd, float a, float b, int lane) {
  __syncthreads();
  sd[lane] = a;
  sd[lane + 64] = b;
  __syncthreads();
  __shared__ float snorm;
  if (lane == 0) {
    float n = 0.f;
    for (int i = 0; i < 128; ++i) n += sd[i] * sd[i];
    snorm = fast_sqrt_f(n) + kFltEps;
  }
  __syncthreads();
  return snorm;
}

__device__ __forceinline__ void descriptor_body(int o, int w, int h, size_t plane, const float *__restrict__ grad,
                                                const KeyRec *__restrict__ kp, const int *__restrict__ range,
                                                const double *__restrict__ angles, const int *__restrict__ nang,
                                                const int *__restrict__ row0, float *__restrict__ table, int capacity,
                                                int block, int nblocks) {
  __shared__ float swm[64], srx[64], sry[64], srt[64];
  __shared__ int sbin[64];  // bx + 8 | (by + 8) << 8 | bt << 16
  __shared__ float sd[128];
  const int lane = threadIdx.x;
  const int lo = range[0], hi = range[1];
  const double xper = ldexp(1.0, o);
  for (int k = lo + block; k < hi; k += nblocks) {
    const KeyRec key = kp[k];
    const double x = key.x / xper, y = key.y / xper, sigma = key.sigma / xper;
    const int xi = (int)(x + 0.5), yi = (int)(y + 0.5);
    const double SBP = 3.0 * sigma + 2.220446049250313e-16;
    const int W = (int)floor(sqrt(2.0) * SBP * 5 / 2.0 + 0.5);
    const int dy0 = max(-W, 1 - yi), dy1 = min(W, h - yi - 2);
    const int dx0 = max(-W, 1 - xi), dx1 = min(W, w - xi - 2);
    const int nx = max(dx1 - dx0 + 1, 0), npx = max(dy1 - dy0 + 1, 0) * nx;
    const float *g = grad + (size_t)key.s * plane * 2;
    const int na = nang[k];
    for (int q = 0; q < na; ++q) {
      const double angle0 = angles[(size_t)k * 4 + q];
      const double st0 = sin(angle0), ct0 = cos(angle0);
      float d0 = 0.f, d1 = 0.f;
      for (int p0 = 0; p0 < npx; p0 += 64) {
        const int p = p0 + lane;
        int code = -1;
        float wm = 0, rbx = 0, rby = 0, rbt = 0;
        if (p < npx) {
          const int px = xi + dx0 + p % nx, py = yi + dy0 + p / nx;
          const float *gp = g + ((size_t)py * w + px) * 2;
          const float mod = gp[0], ang = gp[1];
          const float theta = mod2pi_f((float)((double)ang - angle0));
          const float dx = (float)((double)px - x), dy = (float)((double)py - y);
          const float nxf = (float)((ct0 * dx + st0 * dy) / SBP);
          const float nyf = (float)((-st0 * dx + ct0 * dy) / SBP);
          const float nt = (float)((double)(8.f * theta) / (2 * M_PI));
          const float win = (float)fast_expn(kExpn, (double)(nxf * nxf + nyf * nyf) / 8.0);
          const int bx = (int)floorf((float)((double)nxf - 0.5));
          const int by = (int)floorf((float)((double)nyf - 0.5));
          const int bt = (int)floorf(nt);
          rbx = (float)((double)nxf - (bx + 0.5));
          rby = (float)((double)nyf - (by + 0.5));
          rbt = nt - (float)bt;
          wm = win * mod;
          // pixels whose lower-left bin is outside [-3, 2) reach no bin; keep the code in range
          if (bx >= -3 && bx <= 1 && by >= -3 && by <= 1) code = (bx + 8) | ((by + 8) << 8) | (bt << 16);
        }
        // only the pixels that reach a bin go to LDS, packed in lane (= raster) order: about a third
        // of the window, the rest lies outside the rotated 4 x 4 footprint
        const uint64_t live = __ballot(code >= 0);
        __syncthreads();
        if (code >= 0) {
          const int slot = __popcll(live & ((1ull << lane) - 1));
          sbin[slot] = code;
          swm[slot] = wm;
          srx[slot] = rbx;
          sry[slot] = rby;
          srt[slot] = rbt;
        }
        __syncthreads();
        const int m = __popcll(live);
        for (int r = 0; r < m; ++r) {
          const int c = sbin[r];
          const int bx = (c & 0xff) - 8, by = ((c >> 8) & 0xff) - 8, bt = c >> 16;
          const float a = bin_weight(lane, swm[r], srx[r], sry[r], srt[r], bx, by, bt);
          if (a >= 0.f) d0 += a;
          const float b = bin_weight(lane + 64, swm[r], srx[r], sry[r], srt[r], bx, by, bt);
          if (b >= 0.f) d1 += b;
        }
      }
      float nrm = block_norm(sd, d0, d1, lane);
      d0 /= nrm;
      d1 /= nrm;
      if ((double)d0 > 0.2) d0 = 0.2f;
      if ((double)d1 > 0.2) d1 = 0.2f;
      nrm = block_norm(sd, d0, d1, lane);
      d0 /= nrm;
      d1 /= nrm;
      const long long row = (long long)row0[k] + q;
      if (row < capacity) {
        float *out = table + row * 132;
        if (lane == 0) {
          out[0] = key.x;
          out[1] = key.y;
          out[2] = key.sigma;
          out[3] = (float)angle0;
        }
        out[4 + lane] = (float)(uint8_t)fminf(512.f * d0, 255.f);
        out[4 + 64 + lane] = (float)(uint8_t)fminf(512.f * d1, 255.f);
      }
    }
  }
}
__global__ __launch_bounds__(64) void sift_descriptor_kernel(int o, int w, int h, size_t plane,
                                                             const float *__restrict__ grad,
                                                             const KeyRec *__restrict__ kp,
                                                             const int *__restrict__ range,
                                                             const double *__restrict__ angles,
                                                             const int *__restrict__ nang,
                                                             const int *__restrict__ row0, float *__restrict__ table,
                                                             int capacity) {
  descriptor_body(o, w, h, plane, grad, kp, range, angles, nang, row0, table, capacity, blockIdx.x, gridDim.x);
}

__global__ void sift_count_kernel(const int *__restrict__ ctr, int *__restrict__ count) { *count = ctr[C_NROW]; }

// ---- many images in one chain of launches -----------------------------------------------------------
// The host walks the octaves once for a group of images; every launch has the image as one more grid
// dimension, its extent that of the group's largest image at that octave.  An image's record says where
// its slice of the workspace lies (the pieces of sift_layout); whether the image takes part in octave o,
// and with which w and h, is decided here from wid, hgt and noct.  Blocks outside their image's extent,
// and all blocks of an image that sits out, return at once and together.
struct SiftImg {
  const float *im;
  int *ctr;
  float *L;
  char *scratch;  // the smoothing temporary, the candidates and the gradients, each from its start
  int *cflag, *coff;
  KeyRec *crec;
  int *rowcnt, *rowoff;
  KeyRec *kp;
  double *ang;
  int *nang, *krow;
  float *table;  // the image's region of the caller's table, `capacity` rows
  int *count;
  size_t N;
  int wid, hgt, noct, capacity;
};

struct ImgOctave {
  int w, h;
  bool pyr, det;  // takes part in the pyramid; and in detection and description
};
__host__ __device__ __forceinline__ ImgOctave img_octave(int wid, int hgt, int noct, int o) {
  ImgOctave q;
  q.w = o < 0 ? 2 * wid : wid >> o;
  q.h = o < 0 ? 2 * hgt : hgt >> o;
  q.pyr = o < -1 + noct;
  q.det = q.pyr && q.w >= 3 && q.h >= 3;
  return q;
}
__device__ __forceinline__ ImgOctave img_octave(const SiftImg &r, int o) { return img_octave(r.wid, r.hgt, r.noct, o); }

__global__ __launch_bounds__(256) void sift_batch_init_kernel(const SiftImg *__restrict__ imgs, int nimg) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nimg) return;
  for (int k = 0; k < C_COUNT; ++k) imgs[i].ctr[k] = 0;
}

// grid (columns / 256, rows, images) of the largest image
__global__ __launch_bounds__(256) void sift_batch_upsample_kernel(const SiftImg *__restrict__ imgs) {
  const SiftImg &r = imgs[blockIdx.z];
  if ((int)blockIdx.y >= 2 * r.hgt) return;  // octave -1: every image takes part
  upsample_body(r.im, r.wid, r.hgt, r.L, blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y);
}

__global__ __launch_bounds__(256) void sift_batch_downsample_kernel(const SiftImg *__restrict__ imgs, int o) {
  const SiftImg &r = imgs[blockIdx.z];
  const ImgOctave q = img_octave(r, o);
  if (!q.pyr || (int)blockIdx.y >= q.h) return;
  const int pw = img_octave(r, o - 1).w;
  downsample_body(r.L + 3 * r.N, pw, r.L, q.w, blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y);
}

// VERT: level `level` -> the temporary; else the temporary -> level `level`
template <bool VERT>
__global__ __launch_bounds__(256) void sift_batch_smooth_kernel(const SiftImg *__restrict__ imgs, int o, int level, Taps tp) {
  const SiftImg &r = imgs[blockIdx.z];
  const ImgOctave q = img_octave(r, o);
  if (!q.pyr || (int)blockIdx.y >= q.h) return;
  float *lv = r.L + level * r.N, *tmp = reinterpret_cast<float *>(r.scratch);
  smooth_body<VERT>(VERT ? lv : tmp, VERT ? tmp : lv, q.w, q.h, tp, blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y);
}

// grid (DoG rows / 4, images)
template <bool WRITE>
__global__ __launch_bounds__(256) void sift_batch_extrema_kernel(const SiftImg *__restrict__ imgs, int o) {
  const SiftImg &r = imgs[blockIdx.y];
  const ImgOctave q = img_octave(r, o);
  if (!q.det) return;
  extrema_body<WRITE>(Octave{r.L, r.N, q.w, q.h}, r.rowcnt, r.rowoff, reinterpret_cast<uint32_t *>(r.scratch),
                      blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
}

// One workgroup per image.  STAGE 0: the rows' extrema counts -> offsets and the candidate count; 1: the
// candidates' flags -> keypoint offsets and the octave's keypoint range; 2: the keypoints' angle counts
// -> table rows, after the rows of the image's earlier octaves.
template <int STAGE>
__global__ __launch_bounds__(kScanThreads) void sift_batch_scan_kernel(const SiftImg *__restrict__ imgs, int o) {
  const SiftImg &r = imgs[blockIdx.x];
  const ImgOctave q = img_octave(r, o);
  if (!q.det) return;  // the whole workgroup: no barrier is reached by part of it
  if (STAGE == 0) scan_body(r.rowcnt, 3 * (q.h - 2), nullptr, nullptr, r.rowoff, nullptr, r.ctr + C_NCAND, nullptr);
  if (STAGE == 1)
    scan_body(r.cflag, (int)((size_t)q.w * q.h), r.ctr + C_NCAND, nullptr, r.coff, nullptr, nullptr, r.ctr + C_KP_LO);
  if (STAGE == 2) scan_body(r.nang, 0, nullptr, r.ctr + C_KP_LO, r.krow, r.ctr + C_NROW, nullptr, nullptr);
}

// grid (the image's share of the persistent blocks, images)
__global__ __launch_bounds__(256) void sift_batch_refine_kernel(const SiftImg *__restrict__ imgs, int o, double sigma0) {
  const SiftImg &r = imgs[blockIdx.y];
  const ImgOctave q = img_octave(r, o);
  if (!q.det) return;
  refine_body(Octave{r.L, r.N, q.w, q.h}, o, sigma0, reinterpret_cast<const uint32_t *>(r.scratch), r.ctr + C_NCAND,
              r.cflag, r.crec, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x);
}

__global__ __launch_bounds__(256) void sift_batch_scatter_kernel(const SiftImg *__restrict__ imgs, int o) {
  const SiftImg &r = imgs[blockIdx.y];
  if (!img_octave(r, o).det) return;
  scatter_body(r.ctr + C_NCAND, r.cflag, r.coff, r.crec, r.kp, blockIdx.x * blockDim.x + threadIdx.x,
               gridDim.x * blockDim.x);
}

// grid (columns / 256, rows, images); the three levels in turn
__global__ __launch_bounds__(256) void sift_batch_gradient_kernel(const SiftImg *__restrict__ imgs, int o) {
  const SiftImg &r = imgs[blockIdx.z];
  const ImgOctave q = img_octave(r, o);
  if (!q.det || (int)blockIdx.y >= q.h) return;
  const Octave oc{r.L, r.N, q.w, q.h};
  for (int s = 0; s < 3; ++s)
    gradient_body(oc, reinterpret_cast<float *>(r.scratch), blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y, s);
}

// grid (the image's share of the keypoint blocks, images)
__global__ __launch_bounds__(64) void sift_batch_orientation_kernel(const SiftImg *__restrict__ imgs, int o) {
  const SiftImg &r = imgs[blockIdx.y];
  const ImgOctave q = img_octave(r, o);
  if (!q.det) return;
  orientation_body(o, q.w, q.h, r.N, reinterpret_cast<const float *>(r.scratch), r.kp, r.ctr + C_KP_LO, r.ang, r.nang,
                   blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(64) void sift_batch_descriptor_kernel(const SiftImg *__restrict__ imgs, int o) {
  const SiftImg &r = imgs[blockIdx.y];
  const ImgOctave q = img_octave(r, o);
  if (!q.det) return;
  descriptor_body(o, q.w, q.h, r.N, reinterpret_cast<const float *>(r.scratch), r.kp, r.ctr + C_KP_LO, r.ang, r.nang,
                  r.krow, r.table, r.capacity, blockIdx.x, gridDim.x);
}

__global__ __launch_bounds__(256) void sift_batch_count_kernel(const SiftImg *__restrict__ imgs, int nimg) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nimg) *imgs[i].count = imgs[i].ctr[C_NROW];
}

// Rows cap_off[i] + r of the regions -> rows seg_off[i] + r of the packed outputs: 32 lanes per row, as
// sift_split_kernel (adapter.hip) and with its values.  offs = cap_off[nimg] then seg_off[nimg + 1].
__global__ __launch_bounds__(256) void sift_batch_pack_kernel(const long long *__restrict__ offs, int nimg,
                                                              const float *__restrict__ table, float *__restrict__ packed,
                                                              float *__restrict__ geom, uint8_t *__restrict__ desc) {
  const long long *cap_off = offs, *seg_off = offs + nimg;
  const long long gt = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long row = gt >> 5;
  const int j = (int)(gt & 31);
  if (row >= seg_off[nimg]) return;
  int lo = 0, hi = nimg - 1;  // the last image whose segment starts at or before row (empty segments skipped)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (seg_off[mid] <= row) lo = mid;
    else hi = mid - 1;
  }
  const float *src = table + (size_t)(cap_off[lo] + (row - seg_off[lo])) * 132;
  if (packed)
    for (int c = j; c < 132; c += 32) packed[(size_t)row * 132 + c] = src[c];
  if (geom && j < 4) geom[(size_t)row * 4 + j] = src[j];
  if (desc) {
    const float *d = src + 4 + 4 * j;
    const uint32_t pk = ((uint32_t)(int)d[0] & 0xFFu) | (((uint32_t)(int)d[1] & 0xFFu) << 8) |
                        (((uint32_t)(int)d[2] & 0xFFu) << 16) | (((uint32_t)(int)d[3] & 0xFFu) << 24);
    reinterpret_cast<uint32_t *>(desc)[(size_t)row * 32 + j] = pk;
  }
}

// ---- host side -----------------------------------------------------------------------------------

Taps make_taps(double sigma) {
  Taps t{};
  t.W = std::max((int)std::ceil(4.0 * sigma), 1);
  float acc = 0.f;
  for (int j = 0; j < 2 * t.W + 1; ++j) {
    const float d = (float)(j - t.W) / (float)sigma;
    t.t[j] = (float)std::exp(-0.5 * (double)(d * d));
    acc += t.t[j];
  }
  for (int j = 0; j < 2 * t.W + 1; ++j) t.t[j] /= acc;
  return t;
}

struct SiftLayout {
  size_t N;  // octave -1 area: bounds every octave's candidates and keypoints
  size_t o_ctr, o_L, o_scratch, o_cflag, o_coff, o_crec, o_rowcnt, o_rowoff, o_kp, o_ang, o_nang, o_row, total;
};

// The scratch region holds, one after another on the stream, the smoothing temporary (pyramid), the
// candidate lists (detection) and the gradients (description): none outlives its stage.
SiftLayout sift_layout(int wid, int hgt) {
  SiftLayout l{};
  l.N = (size_t)(2 * wid) * (size_t)(2 * hgt);
  const size_t rows = 3 * (size_t)(2 * hgt);
  WsWalk w, det;  // det: the detection lists inside the scratch region (cand at 0)
  l.o_ctr = w.reserve(C_COUNT * sizeof(int));
  l.o_L = w.reserve(6 * l.N * sizeof(float));
  det.reserve(l.N * sizeof(uint32_t));
  l.o_cflag = det.reserve(l.N * sizeof(int));
  l.o_coff = det.reserve(l.N * sizeof(int));
  l.o_crec = det.reserve(l.N * sizeof(KeyRec));
  l.o_scratch = w.reserve(std::max({det.end(), 6 * l.N * sizeof(float), l.N * sizeof(float)}));
  l.o_rowcnt = w.reserve(rows * sizeof(int));
  l.o_rowoff = w.reserve(rows * sizeof(int));
  l.o_kp = w.reserve(l.N * sizeof(KeyRec));
  l.o_ang = w.reserve(l.N * 4 * sizeof(double));
  l.o_nang = w.reserve(l.N * sizeof(int));
  l.o_row = w.reserve(l.N * sizeof(int));
  l.total = w.end();
  return l;
}

}  // namespace

// O = max(floor(log2(min(w, h))) - omin - 3, 1) with omin = -1
int sift_noctaves(int wid, int hgt) {
  return std::max((int)std::floor(std::log2((double)std::min(wid, hgt))) + 1 - 3, 1);
}

int sift_check(int wid, int hgt) {
  if (wid <= 0 || hgt <= 0) return set_error(SPV_ERR_INVALID, "bad image size %d x %d", wid, hgt);
  if (wid > kSiftMaxSide || hgt > kSiftMaxSide)
    return set_error(SPV_ERR_INVALID, "image %d x %d: each side must be at most %d", wid, hgt, kSiftMaxSide);
  return SPV_OK;
}

size_t sift_workspace_bytes(int wid, int hgt) { return sift_layout(wid, hgt).total; }

int sift_run(const float *d_im, int wid, int hgt, void *d_ws, size_t ws_bytes, float *d_table, int capacity,
             int *d_count, hipStream_t st) {
  SPV_TRY(sift_check(wid, hgt));
  if (!d_im || !d_ws || !d_count || (capacity > 0 && !d_table)) return set_error(SPV_ERR_INVALID, "null pointer");
  if (capacity < 0) return set_error(SPV_ERR_INVALID, "negative capacity");
  const SiftLayout l = sift_layout(wid, hgt);
  if (ws_bytes < l.total) return set_error(SPV_ERR_INVALID, "workspace %zu bytes, need %zu", ws_bytes, l.total);
  char *ws = static_cast<char *>(d_ws);
  int *ctr = reinterpret_cast<int *>(ws + l.o_ctr);
  float *L = reinterpret_cast<float *>(ws + l.o_L);
  char *scratch = ws + l.o_scratch;
  float *tmp = reinterpret_cast<float *>(scratch);
  uint32_t *cand = reinterpret_cast<uint32_t *>(scratch);
  int *cflag = reinterpret_cast<int *>(scratch + l.o_cflag);
  int *coff = reinterpret_cast<int *>(scratch + l.o_coff);
  KeyRec *crec = reinterpret_cast<KeyRec *>(scratch + l.o_crec);
  float *grad = reinterpret_cast<float *>(scratch);
  int *rowcnt = reinterpret_cast<int *>(ws + l.o_rowcnt);
  int *rowoff = reinterpret_cast<int *>(ws + l.o_rowoff);
  KeyRec *kp = reinterpret_cast<KeyRec *>(ws + l.o_kp);
  double *ang = reinterpret_cast<double *>(ws + l.o_ang);
  int *nang = reinterpret_cast<int *>(ws + l.o_nang);
  int *krow = reinterpret_cast<int *>(ws + l.o_row);
  SPV_HIP_CHECK(hipMemsetAsync(ctr, 0, C_COUNT * sizeof(int), st));

  const double sigmak = std::pow(2.0, 1.0 / 3), sigma0 = 1.6 * sigmak;
  const double dsigma0 = sigma0 * std::sqrt(1.0 - 1.0 / (sigmak * sigmak));
  Taps level_taps[5];
  for (int s = 0; s < 5; ++s) level_taps[s] = make_taps(dsigma0 * std::pow(sigmak, s));
  const double sa = sigma0 * std::pow(sigmak, -1), sb = 0.5 * 2.0;
  const Taps first_taps = make_taps(std::sqrt(sa * sa - sb * sb));

  auto smooth = [&](const float *in, float *out, int w, int h, const Taps &t) -> int {
    const dim3 grid((w + 255) / 256, h);
    {
      ProfScope ps("sift_pyramid", st);
      sift_smooth_kernel<true><<<grid, 256, 0, st>>>(in, tmp, w, h, t);
      sift_smooth_kernel<false><<<grid, 256, 0, st>>>(tmp, out, w, h, t);
    }
    SPV_HIP_CHECK(hipGetLastError());
    return SPV_OK;
  };

  const int O = sift_noctaves(wid, hgt);
  int pw = 0;
  for (int o = -1; o < -1 + O; ++o) {
    const int w = o < 0 ? 2 * wid : wid >> o, h = o < 0 ? 2 * hgt : hgt >> o;
    const size_t plane = (size_t)w * h;
    {
      ProfScope ps("sift_pyramid", st);
      if (o < 0) sift_upsample_kernel<<<dim3((2 * wid + 255) / 256, 2 * hgt), 256, 0, st>>>(d_im, wid, hgt, L);
      else sift_downsample_kernel<<<dim3((w + 255) / 256, h), 256, 0, st>>>(L + 3 * l.N, pw, L, w);
    }
    SPV_HIP_CHECK(hipGetLastError());
    // level buffers keep a stride of N so that level 2 survives as the next octave's source
    if (o < 0) SPV_TRY(smooth(L, L, w, h, first_taps));
    for (int s = 0; s < 5; ++s) SPV_TRY(smooth(L + s * l.N, L + (s + 1) * l.N, w, h, level_taps[s]));
    pw = w;
    if (w < 3 || h < 3) continue;  // no DoG interior: no keypoints
    Octave oc{L, l.N, w, h};
    const int rows = 3 * (h - 2);
    {
      ProfScope ps("sift_detect", st);
      sift_extrema_kernel<false><<<(rows + 3) / 4, 256, 0, st>>>(oc, rowcnt, nullptr, nullptr);
      sift_scan_kernel<<<1, kScanThreads, 0, st>>>(rowcnt, rows, nullptr, nullptr, rowoff, nullptr, ctr + C_NCAND,
                                                   nullptr);
      sift_extrema_kernel<true><<<(rows + 3) / 4, 256, 0, st>>>(oc, nullptr, rowoff, cand);
      const int rblocks = (int)std::min<size_t>((plane + 255) / 256, kPersistBlocks);
      sift_refine_kernel<<<rblocks, 256, 0, st>>>(oc, o, sigma0, cand, ctr + C_NCAND, cflag, crec);
      // the octave's keypoints, from index 0: orientation and descriptor use one octave at a time
      sift_scan_kernel<<<1, kScanThreads, 0, st>>>(cflag, (int)plane, ctr + C_NCAND, nullptr, coff, nullptr,
                                                   nullptr, ctr + C_KP_LO);
      sift_scatter_kernel<<<rblocks, 256, 0, st>>>(ctr + C_NCAND, cflag, coff, crec, kp);
    }
    SPV_HIP_CHECK(hipGetLastError());
    {
      ProfScope ps("sift_describe", st);
      sift_gradient_kernel<<<dim3((w + 255) / 256, h, 3), 256, 0, st>>>(Octave{L, l.N, w, h}, grad);
      sift_orientation_kernel<<<kKeyBlocks, 64, 0, st>>>(o, w, h, l.N, grad, kp, ctr + C_KP_LO, ang, nang);
      sift_scan_kernel<<<1, kScanThreads, 0, st>>>(nang, 0, nullptr, ctr + C_KP_LO, krow, ctr + C_NROW, nullptr,
                                                   nullptr);
      sift_descriptor_kernel<<<kKeyBlocks, 64, 0, st>>>(o, w, h, l.N, grad, kp, ctr + C_KP_LO, ang, nang, krow,
                                                        d_table, capacity);
    }
    SPV_HIP_CHECK(hipGetLastError());
  }
  sift_count_kernel<<<1, 1, 0, st>>>(ctr, d_count);
  SPV_HIP_CHECK(hipGetLastError());
  return SPV_OK;
}

// ---- many images in one chain of launches: host side ------------------------------------------------

int sift_batch_plan(const int32_t *sizes, int nimg, size_t ws_bytes, SiftBatchPlan *p) {
  if (nimg < 0) return set_error(SPV_ERR_INVALID, "negative image count");
  if (nimg > 0 && !sizes) return set_error(SPV_ERR_INVALID, "null sizes");
  SiftBatchPlan q;
  std::vector<size_t> need((size_t)nimg);
  for (int i = 0; i < nimg; ++i) {
    SPV_TRY(sift_check(sizes[2 * i], sizes[2 * i + 1]));
    need[i] = sift_layout(sizes[2 * i], sizes[2 * i + 1]).total;
    q.min_bytes = std::max(q.min_bytes, need[i]);
    q.pixels += (long long)sizes[2 * i] * sizes[2 * i + 1];
  }
  if (ws_bytes && ws_bytes < q.min_bytes)
    return set_error(SPV_ERR_INVALID, "workspace %zu bytes, the largest image alone needs %zu", ws_bytes, q.min_bytes);
  // the images in order; a group is closed when the next slice would not fit, or at kSiftBatchMaxImages
  auto cut = [&](size_t cap, std::vector<std::pair<int, int>> *groups) {
    size_t most = 0, sum = 0;
    int first = 0;
    for (int i = 0; i < nimg; ++i) {
      if (i > first && ((cap && sum + need[i] > cap) || i - first == kSiftBatchMaxImages)) {
        if (groups) groups->emplace_back(first, i - first);
        first = i;
        sum = 0;
      }
      sum += need[i];
      most = std::max(most, sum);
    }
    if (nimg > 0 && groups) groups->emplace_back(first, nimg - first);
    return most;
  };
  q.all_bytes = cut(0, nullptr);
  cut(ws_bytes, &q.groups);
  *p = std::move(q);
  return SPV_OK;
}

namespace {

constexpr int kPersistFloor = 32, kKeyFloor = 128;  // the least share of the persistent grids an image of a large group gets

// One group: images [first, first + n), their slices one after another from d_ws; d_imgs holds their records.
int sift_batch_group(const SiftImg *d_imgs, const int32_t *sizes, int n, hipStream_t st) {
  const double sigmak = std::pow(2.0, 1.0 / 3), sigma0 = 1.6 * sigmak;
  const double dsigma0 = sigma0 * std::sqrt(1.0 - 1.0 / (sigmak * sigmak));
  Taps level_taps[5];
  for (int s = 0; s < 5; ++s) level_taps[s] = make_taps(dsigma0 * std::pow(sigmak, s));
  const double sa = sigma0 * std::pow(sigmak, -1), sb = 0.5 * 2.0;
  const Taps first_taps = make_taps(std::sqrt(sa * sa - sb * sb));

  sift_batch_init_kernel<<<(n + 255) / 256, 256, 0, st>>>(d_imgs, n);
  SPV_HIP_CHECK(hipGetLastError());
  int O = 1;
  for (int i = 0; i < n; ++i) O = std::max(O, sift_noctaves(sizes[2 * i], sizes[2 * i + 1]));
  for (int o = -1; o < -1 + O; ++o) {
    // the grid's extent: the widest and the tallest image that takes part (they need not be the same one)
    int pw = 0, ph = 0, dw = 0, dh = 0;
    size_t dplane = 0;
    for (int i = 0; i < n; ++i) {
      const ImgOctave q = img_octave(sizes[2 * i], sizes[2 * i + 1], sift_noctaves(sizes[2 * i], sizes[2 * i + 1]), o);
      if (q.pyr) pw = std::max(pw, q.w), ph = std::max(ph, q.h);
      if (q.det) dw = std::max(dw, q.w), dh = std::max(dh, q.h), dplane = std::max(dplane, (size_t)q.w * q.h);
    }
    const dim3 pgrid((pw + 255) / 256, ph, n);
    auto smooth = [&](int from, int to, const Taps &t) -> int {
      ProfScope ps("sift_batch_pyramid", st);
      sift_batch_smooth_kernel<true><<<pgrid, 256, 0, st>>>(d_imgs, o, from, t);
      sift_batch_smooth_kernel<false><<<pgrid, 256, 0, st>>>(d_imgs, o, to, t);
      SPV_HIP_CHECK(hipGetLastError());
      return SPV_OK;
    };
    {
      ProfScope ps("sift_batch_pyramid", st);
      if (o < 0) sift_batch_upsample_kernel<<<pgrid, 256, 0, st>>>(d_imgs);
      else sift_batch_downsample_kernel<<<pgrid, 256, 0, st>>>(d_imgs, o);
    }
    SPV_HIP_CHECK(hipGetLastError());
    if (o < 0) SPV_TRY(smooth(0, 0, first_taps));
    for (int s = 0; s < 5; ++s) SPV_TRY(smooth(s, s + 1, level_taps[s]));
    if (dplane == 0) continue;  // no image of the group has a DoG interior at this octave
    const int rows = 3 * (dh - 2);
    const dim3 egrid((rows + 3) / 4, n);
    const dim3 rgrid((unsigned)std::min<size_t>((dplane + 255) / 256, std::max(kPersistBlocks / n, kPersistFloor)), n);
    const dim3 kgrid(std::max(kKeyBlocks / n, kKeyFloor), n);
    {
      ProfScope ps("sift_batch_detect", st);
      sift_batch_extrema_kernel<false><<<egrid, 256, 0, st>>>(d_imgs, o);
      sift_batch_scan_kernel<0><<<n, kScanThreads, 0, st>>>(d_imgs, o);
      sift_batch_extrema_kernel<true><<<egrid, 256, 0, st>>>(d_imgs, o);
      sift_batch_refine_kernel<<<rgrid, 256, 0, st>>>(d_imgs, o, sigma0);
      sift_batch_scan_kernel<1><<<n, kScanThreads, 0, st>>>(d_imgs, o);
      sift_batch_scatter_kernel<<<rgrid, 256, 0, st>>>(d_imgs, o);
    }
    SPV_HIP_CHECK(hipGetLastError());
    {
      ProfScope ps("sift_batch_describe", st);
      sift_batch_gradient_kernel<<<dim3((dw + 255) / 256, dh, n), 256, 0, st>>>(d_imgs, o);
      sift_batch_orientation_kernel<<<kgrid, 64, 0, st>>>(d_imgs, o);
      sift_batch_scan_kernel<2><<<n, kScanThreads, 0, st>>>(d_imgs, o);
      sift_batch_descriptor_kernel<<<kgrid, 64, 0, st>>>(d_imgs, o);
    }
    SPV_HIP_CHECK(hipGetLastError());
  }
  sift_batch_count_kernel<<<(n + 255) / 256, 256, 0, st>>>(d_imgs, n);
  SPV_HIP_CHECK(hipGetLastError());
  return SPV_OK;
}

// The scratch of a call that returns before its kernels: back to the cache behind them, on every way out.
struct ReleaseAfter {
  DevBuf &b;
  hipStream_t st;
  ~ReleaseAfter() { b.release_after(st); }
};

}  // namespace

int sift_batch_run(const float *d_images, const int32_t *sizes, int nimg, void *d_ws, size_t ws_bytes, float *d_table,
                   const long long *cap_off, int32_t *d_counts, hipStream_t st) {
  SiftBatchPlan plan;
  SPV_TRY(sift_batch_plan(sizes, nimg, ws_bytes, &plan));
  SPV_TRY(check_offsets(cap_off, nimg, "cap_off"));
  if (nimg == 0) return SPV_OK;
  if (!d_images || !d_ws || !d_counts || (cap_off[nimg] > 0 && !d_table)) return set_error(SPV_ERR_INVALID, "null pointer");
  if (ws_bytes < plan.min_bytes)
    return set_error(SPV_ERR_INVALID, "workspace %zu bytes, the largest image alone needs %zu", ws_bytes, plan.min_bytes);
  // the records of all images, one upload; every group's slices start over at d_ws, which stream order allows
  std::vector<SiftImg> imgs((size_t)nimg);
  size_t pix = 0;
  int i = 0;
  for (const auto &g : plan.groups) {
    char *ws = static_cast<char *>(d_ws);
    for (; i < g.first + g.second; ++i) {
      const int wid = sizes[2 * i], hgt = sizes[2 * i + 1];
      const SiftLayout l = sift_layout(wid, hgt);
      char *scratch = ws + l.o_scratch;
      imgs[i] = SiftImg{d_images + pix,
                        reinterpret_cast<int *>(ws + l.o_ctr),
                        reinterpret_cast<float *>(ws + l.o_L),
                        scratch,
                        reinterpret_cast<int *>(scratch + l.o_cflag),
                        reinterpret_cast<int *>(scratch + l.o_coff),
                        reinterpret_cast<KeyRec *>(scratch + l.o_crec),
                        reinterpret_cast<int *>(ws + l.o_rowcnt),
                        reinterpret_cast<int *>(ws + l.o_rowoff),
                        reinterpret_cast<KeyRec *>(ws + l.o_kp),
                        reinterpret_cast<double *>(ws + l.o_ang),
                        reinterpret_cast<int *>(ws + l.o_nang),
                        reinterpret_cast<int *>(ws + l.o_row),
                        d_table + (size_t)cap_off[i] * 132,
                        d_counts + i,
                        l.N,
                        wid,
                        hgt,
                        sift_noctaves(wid, hgt),
                        (int)(cap_off[i + 1] - cap_off[i])};
      pix += (size_t)wid * hgt;
      ws += l.total;
    }
  }
  DevBuf recs;
  SPV_TRY(recs.alloc(imgs.size() * sizeof(SiftImg)));
  ReleaseAfter release{recs, st};
  // (pageable source: the copy has left `imgs` when the call returns)
  SPV_HIP_CHECK(hipMemcpyAsync(recs.p, imgs.data(), imgs.size() * sizeof(SiftImg), hipMemcpyHostToDevice, st));
  for (const auto &g : plan.groups)
    SPV_TRY(sift_batch_group(recs.as<SiftImg>() + g.first, sizes + 2 * (size_t)g.first, g.second, st));
  return SPV_OK;
}

int sift_batch_pack_run(const float *d_table, const long long *cap_off, const long long *seg_off, int nimg,
                        float *d_packed, float *d_geom, uint8_t *d_desc, hipStream_t st) {
  if (nimg < 0) return set_error(SPV_ERR_INVALID, "negative image count");
  SPV_TRY(check_offsets(cap_off, nimg, "cap_off"));
  SPV_TRY(check_offsets(seg_off, nimg, "seg_off"));
  for (int i = 0; i < nimg; ++i)
    if (seg_off[i + 1] - seg_off[i] > cap_off[i + 1] - cap_off[i])
      return set_error(SPV_ERR_INVALID, "segment %d: %lld rows, its region holds %lld", i, seg_off[i + 1] - seg_off[i],
                       cap_off[i + 1] - cap_off[i]);
  if (!d_packed && !d_geom && !d_desc) return set_error(SPV_ERR_INVALID, "no output is wanted");
  const long long total = seg_off[nimg];
  if (total == 0) return SPV_OK;
  if (!d_table) return set_error(SPV_ERR_INVALID, "null pointer");
  std::vector<long long> offs(cap_off, cap_off + nimg);
  offs.insert(offs.end(), seg_off, seg_off + nimg + 1);
  DevBuf tab;
  SPV_TRY(tab.alloc(offs.size() * sizeof(long long)));
  ReleaseAfter release{tab, st};
  // (pageable source: the copy has left `offs` when the call returns)
  SPV_HIP_CHECK(hipMemcpyAsync(tab.p, offs.data(), offs.size() * sizeof(long long), hipMemcpyHostToDevice, st));
  ProfScope ps("sift_batch_pack", st);
  sift_batch_pack_kernel<<<(unsigned)((total * 32 + 255) / 256), 256, 0, st>>>(tab.as<long long>(), nimg, d_table, d_packed,
                                                                               d_geom, d_desc);
  SPV_HIP_CHECK(hipGetLastError());
  return SPV_OK;
}

}  // namespace spv
