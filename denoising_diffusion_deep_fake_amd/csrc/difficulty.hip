// balance_training_images: the scoring epoch's device side (d3f/balance_training_images/lit_module.py:122-193).
//
//   l1_per_image_scatter   compute_difficulty_loss (:137-140) written to scores[index[b]]: the partial stage IS
//                          l1_per_image's (loss.hip: L1_PARTS float64 partials per image), the last stage adds them in
//                          the same order through the same device function -- the value is l1_per_image's bit for bit
//   difficulty_classes     compute_difficulty_index_for_each_loss (:181-193) over a score buffer in which NaN means
//                          "not scored": min / max (order-free), then per entry the reference's fp32 operations one by
//                          one -- q = (s - min) / (max - min) (IEEE subtract, IEEE divide, no reciprocal, no contraction),
//                          q = min(max(q, 0), 0.99999f), class = (int64)(q * (float)classes) -- and the class counts
//                          (integer adds: the result does not depend on the launch geometry).  max == min: class 0 (the
//                          reference divides 0 by 0 there and ends at INT64_MIN; a deliberate difference)
//   difficulty_histogram   what axes.hist(difficulty_index) (:151-152) computes -- numpy.histogram(x, bins) over the
//                          entries >= 0 -- and a chart of it with a fixed integer geometry (include/d3f_hip.h)
//
// Every pass is a grid-stride partial pass (at most DIFF_BLOCKS blocks, one partial each) followed by a pass in which
// every block folds the partials itself (min and max do not depend on the order) and goes on: no host round trip, no
// grid barrier.  Counts are kept in LDS per block and flushed with one global atomicAdd per bin and block when they fit
// (DIFF_LDS_BINS), else added straight to global memory.
#include "common.h"
#include "pointwise.h"

namespace d3f {

constexpr int DIFF_THREADS = 256;
constexpr int DIFF_BLOCKS = 256;      // partials per pass
constexpr int DIFF_LDS_BINS = 2048;   // counts of up to this many bins are gathered in LDS first (8 KB)
constexpr int DIFF_MAX_CLASSES = 65536;
constexpr int CHART_MAX_EXTENT = 16384;

static inline int diff_blocks(long n) {
  const long b = (n + DIFF_THREADS * 4 - 1) / (DIFF_THREADS * 4);
  return (int)(b < 1 ? 1 : (b > DIFF_BLOCKS ? DIFF_BLOCKS : b));
}

// ---- 1. per-image L1, scattered ---------------------------------------------------------------------------------------
__global__ void l1_scatter_finalize_kernel(const double* __restrict__ partial, const int64_t* __restrict__ index,
                                           float* __restrict__ scores, int N, int B, long per_image) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const int64_t dst = index[b];
  if (dst < 0 || dst >= (int64_t)N) return;  // outside the buffer: nothing is written
  scores[dst] = l1_image_mean(partial, b, per_image);
}

int l1_per_image_scatter_launch(const float* pred, const float* target, const int64_t* index, float* scores, int N,
                                void* workspace, int B, long per_image, hipStream_t stream) {
  if (B == 0) return 0;
  double* partial = reinterpret_cast<double*>(workspace);
  if (int rc = l1_partials_launch(pred, target, partial, B, per_image, stream)) return rc;
  hipLaunchKernelGGL(l1_scatter_finalize_kernel, dim3((B + 63) / 64), dim3(64), 0, stream, partial, index, scores, N, B,
                     per_image);
  D3F_HIP(hipGetLastError());
  return 0;
}

// ---- block-wide folds -------------------------------------------------------------------------------------------------
template <typename T> struct MinMax {
  T lo, hi;
};
// lo = min, hi = max over the block; every thread gets the result.  red: 2 * DIFF_THREADS elements of LDS
template <typename T, typename FMin, typename FMax>
__device__ __forceinline__ MinMax<T> block_minmax(T lo, T hi, T* red, FMin fmin_, FMax fmax_) {
  const int t = threadIdx.x;
  red[t] = lo;
  red[DIFF_THREADS + t] = hi;
  __syncthreads();
  for (int o = DIFF_THREADS / 2; o > 0; o >>= 1) {
    if (t < o) {
      red[t] = fmin_(red[t], red[t + o]);
      red[DIFF_THREADS + t] = fmax_(red[DIFF_THREADS + t], red[DIFF_THREADS + t + o]);
    }
    __syncthreads();
  }
  const MinMax<T> r{red[0], red[DIFF_THREADS]};
  __syncthreads();  // red may be used again
  return r;
}
__device__ __forceinline__ float f_min(float a, float b) { return fminf(a, b); }  // a NaN operand is passed over
__device__ __forceinline__ float f_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ long long i_min(long long a, long long b) { return a < b ? a : b; }
__device__ __forceinline__ long long i_max(long long a, long long b) { return a > b ? a : b; }

// counts of one block: LDS bins flushed once, or global adds.  `bin` outside [0, bins) is never counted.
struct BinCounter {
  int32_t* lds;  // null: straight to global
  int32_t* global;
  int bins;
  __device__ __forceinline__ void add(long long bin) const {
    if (bin < 0 || bin >= (long long)bins) return;
    atomicAdd(lds != nullptr ? &lds[bin] : &global[bin], 1);
  }
};
__device__ __forceinline__ BinCounter bin_counter_begin(int32_t* lds, int32_t* global, int bins) {
  const bool use_lds = bins <= DIFF_LDS_BINS;
  if (use_lds) {
    for (int i = threadIdx.x; i < bins; i += DIFF_THREADS) lds[i] = 0;
    __syncthreads();
  }
  return BinCounter{use_lds ? lds : nullptr, global, bins};
}
__device__ __forceinline__ void bin_counter_end(const BinCounter& c) {
  if (c.lds == nullptr) return;
  __syncthreads();
  for (int i = threadIdx.x; i < c.bins; i += DIFF_THREADS) {
    const int32_t v = c.lds[i];
    if (v != 0) atomicAdd(&c.global[i], v);
  }
}

// ---- 2. classes ---------------------------------------------------------------------------------------------------------
// partial[block] = {min, max} over the block's scored (non-NaN) entries, {+inf, -inf} when it saw none; counts zeroed
__global__ __launch_bounds__(DIFF_THREADS) void score_minmax_partial_kernel(const float* __restrict__ scores, int N,
                                                                            float* __restrict__ partial,
                                                                            int32_t* __restrict__ counts, int bins) {
  __shared__ float red[2 * DIFF_THREADS];
  const long stride = (long)gridDim.x * DIFF_THREADS, first = (long)blockIdx.x * DIFF_THREADS + threadIdx.x;
  for (long i = first; i < bins; i += stride) counts[i] = 0;
  float lo = INFINITY, hi = -INFINITY;
  for (long i = first; i < N; i += stride) {
    const float s = scores[i];
    lo = fminf(lo, s);
    hi = fmaxf(hi, s);
  }
  const MinMax<float> r = block_minmax(lo, hi, red, f_min, f_max);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = r.lo;
    partial[2 * blockIdx.x + 1] = r.hi;
  }
}

__global__ __launch_bounds__(DIFF_THREADS) void score_classify_kernel(const float* __restrict__ scores, int N,
                                                                      int number_of_classes,
                                                                      const float* __restrict__ partial, int nparts,
                                                                      int64_t* __restrict__ classes,
                                                                      int32_t* __restrict__ counts,
                                                                      float* __restrict__ minmax) {
  __shared__ float red[2 * DIFF_THREADS];
  __shared__ int32_t bins_lds[DIFF_LDS_BINS];
  const int t = threadIdx.x;
  const MinMax<float> r = block_minmax(t < nparts ? partial[2 * t] : INFINITY, t < nparts ? partial[2 * t + 1] : -INFINITY,
                                       red, f_min, f_max);
  const bool any = r.lo <= r.hi;  // {+inf, -inf}: nothing was scored
  if (blockIdx.x == 0 && t == 0) {
    minmax[0] = any ? r.lo : NAN;
    minmax[1] = any ? r.hi : NAN;
  }
  const BinCounter counter = bin_counter_begin(bins_lds, counts, number_of_classes);
  const float range = __fsub_rn(r.hi, r.lo), fc = (float)number_of_classes;
  const bool flat = !(r.hi > r.lo);  // max == min: class 0 for every scored entry
  for (long i = (long)blockIdx.x * DIFF_THREADS + t; i < N; i += (long)gridDim.x * DIFF_THREADS) {
    const float s = scores[i];
    long long c = -1;
    if (s == s) {
      c = 0;
      if (!flat) {
        float q = __fdiv_rn(__fsub_rn(s, r.lo), range);
        q = fminf(fmaxf(q, 0.f), 0.99999f);
        c = (long long)__fmul_rn(q, fc);
      }
      counter.add(c);
    }
    classes[i] = c;
  }
  bin_counter_end(counter);
}

size_t difficulty_classes_workspace_bytes(int N) {
  (void)N;
  return (size_t)DIFF_BLOCKS * 2 * sizeof(float) + 64;
}

int difficulty_classes_launch(const float* scores, int N, int number_of_classes, int64_t* classes, int32_t* counts,
                              float* minmax, void* workspace, hipStream_t stream) {
  D3F_CHECK(N >= 0, "difficulty_classes: N = %d", N);
  D3F_CHECK(number_of_classes >= 1 && number_of_classes <= DIFF_MAX_CLASSES, "difficulty_classes: %d classes outside 1..%d",
            number_of_classes, DIFF_MAX_CLASSES);
  if (N == 0) {  // nothing to score: no kernel; zero counts, NaN min and max (all-ones bytes are a NaN)
    D3F_HIP(hipMemsetAsync(counts, 0, (size_t)number_of_classes * sizeof(int32_t), stream));
    D3F_HIP(hipMemsetAsync(minmax, 0xFF, 2 * sizeof(float), stream));
    return 0;
  }
  float* partial = reinterpret_cast<float*>(workspace);
  const int nparts = diff_blocks(N);
  hipLaunchKernelGGL(score_minmax_partial_kernel, dim3(nparts), dim3(DIFF_THREADS), 0, stream, scores, N, partial, counts,
                     number_of_classes);
  D3F_HIP(hipGetLastError());
  hipLaunchKernelGGL(score_classify_kernel, dim3(diff_blocks(N)), dim3(DIFF_THREADS), 0, stream, scores, N,
                     number_of_classes, partial, nparts, classes, counts, minmax);
  D3F_HIP(hipGetLastError());
  return 0;
}

// ---- 3. histogram and chart -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DIFF_THREADS) void class_minmax_partial_kernel(const int64_t* __restrict__ classes, int N,
                                                                            long long* __restrict__ partial,
                                                                            int32_t* __restrict__ bin_counts, int bins) {
  __shared__ long long red[2 * DIFF_THREADS];
  const long stride = (long)gridDim.x * DIFF_THREADS, first = (long)blockIdx.x * DIFF_THREADS + threadIdx.x;
  for (long i = first; i < bins; i += stride) bin_counts[i] = 0;
  long long lo = INT64_MAX, hi = -1;
  for (long i = first; i < N; i += stride) {
    const long long v = classes[i];
    if (v >= 0) {
      lo = i_min(lo, v);
      hi = i_max(hi, v);
    }
  }
  const MinMax<long long> r = block_minmax(lo, hi, red, i_min, i_max);
  if (threadIdx.x == 0) {
    partial[2 * blockIdx.x] = r.lo;
    partial[2 * blockIdx.x + 1] = r.hi;
  }
}

// numpy.histogram(x, bins) with uniform bins: range (min, max) -- (0, 1) for no data, widened by 0.5 both ways when
// min == max -- edges numpy.linspace(lo, hi, bins + 1): e_k = k * ((hi - lo) / bins) + lo, e_bins = hi
__device__ __forceinline__ double hist_edge(int k, int bins, double lo, double hi, double step) {
  return k == bins ? hi : (double)k * step + lo;
}
__global__ __launch_bounds__(DIFF_THREADS) void class_histogram_kernel(const int64_t* __restrict__ classes, int N, int bins,
                                                                       const long long* __restrict__ partial, int nparts,
                                                                       int32_t* __restrict__ bin_counts,
                                                                       double* __restrict__ range) {
  __shared__ long long red[2 * DIFF_THREADS];
  __shared__ int32_t bins_lds[DIFF_LDS_BINS];
  const int t = threadIdx.x;
  const MinMax<long long> r =
      block_minmax(t < nparts ? partial[2 * t] : (long long)INT64_MAX, t < nparts ? partial[2 * t + 1] : -1LL, red, i_min, i_max);
  double lo = 0.0, hi = 1.0;
  if (r.hi >= 0) {
    lo = (double)r.lo;
    hi = (double)r.hi;
    if (r.lo == r.hi) {
      lo -= 0.5;
      hi += 0.5;
    }
  }
  if (blockIdx.x == 0 && t == 0) {
    range[0] = lo;
    range[1] = hi;
  }
  const BinCounter counter = bin_counter_begin(bins_lds, bin_counts, bins);
  const double width = hi - lo, step = width / (double)bins;
  for (long i = (long)blockIdx.x * DIFF_THREADS + t; i < N; i += (long)gridDim.x * DIFF_THREADS) {
    const long long c = classes[i];
    if (c < 0) continue;
    const double v = (double)c;
    int k = (int)floor((v - lo) / width * (double)bins);
    k = k < 0 ? 0 : (k > bins - 1 ? bins - 1 : k);
    if (v < hist_edge(k, bins, lo, hi, step)) {
      if (k > 0) --k;
    } else if (k < bins - 1 && v >= hist_edge(k + 1, bins, lo, hi, step)) {
      ++k;
    }
    counter.add(k);
  }
  bin_counter_end(counter);
}

struct ChartGeom {
  int H, W, bins;
  int x0, x1, y0, y1;  // the box (frame included)
  int IW, IH;          // its interior
};
static inline ChartGeom chart_geom(int H, int W, int bins) {
  ChartGeom g;
  g.H = H, g.W = W, g.bins = bins;
  g.x0 = W / 8, g.x1 = W - W / 10, g.y0 = H * 3 / 25, g.y1 = H - H * 11 / 100;
  g.IW = (g.x1 - 1) - (g.x0 + 1), g.IH = (g.y1 - 1) - (g.y0 + 1);
  return g;
}

// one lane per pixel: 255 background, the frame 0, bar i over columns [xi0 + i IW / bins, xi0 + (i + 1) IW / bins) and the
// rows [yi1 - h_i, yi1), h_i = counts[i] IH 20 / (cmax 21), in (31, 119, 180)
__global__ __launch_bounds__(DIFF_THREADS) void histogram_chart_kernel(ChartGeom g, const int32_t* __restrict__ bin_counts,
                                                                       uint8_t* __restrict__ chart) {
  __shared__ long long red[2 * DIFF_THREADS];
  long long m = 0;
  for (int i = threadIdx.x; i < g.bins; i += DIFF_THREADS) m = i_max(m, (long long)bin_counts[i]);
  const long long cmax = block_minmax(m, m, red, i_min, i_max).hi;
  const long p = (long)blockIdx.x * DIFF_THREADS + threadIdx.x;
  if (p >= (long)g.H * g.W) return;
  const int y = (int)(p / g.W), x = (int)(p - (long)y * g.W);
  const int xi0 = g.x0 + 1, xi1 = g.x1 - 1, yi0 = g.y0 + 1, yi1 = g.y1 - 1;
  uint8_t cr = 255, cg = 255, cb = 255;
  if (x >= g.x0 && x < g.x1 && y >= g.y0 && y < g.y1) {
    if (x < xi0 || x >= xi1 || y < yi0 || y >= yi1) {
      cr = cg = cb = 0;
    } else if (cmax > 0) {
      const long long dx = x - xi0;
      int i = (int)(dx * g.bins / g.IW);  // i IW / bins <= dx: bar i starts at or left of x
      while (i + 1 < g.bins && (long long)(i + 1) * g.IW / g.bins <= dx) ++i;
      const long long h = (long long)bin_counts[i] * g.IH * 20 / (cmax * 21);
      if ((long long)y >= (long long)yi1 - h) cr = 31, cg = 119, cb = 180;
    }
  }
  uint8_t* o = chart + p * 3;
  o[0] = cr;
  o[1] = cg;
  o[2] = cb;
}

size_t difficulty_histogram_workspace_bytes(int N) {
  (void)N;
  return (size_t)DIFF_BLOCKS * 2 * sizeof(long long) + 64;
}

int difficulty_histogram_u8_launch(const int64_t* classes, int N, int bins, int32_t* bin_counts, double* range,
                                   uint8_t* chart, int H, int W, void* workspace, hipStream_t stream) {
  D3F_CHECK(N >= 0, "difficulty_histogram_u8: N = %d", N);
  D3F_CHECK(H >= 32 && W >= 32 && H <= CHART_MAX_EXTENT && W <= CHART_MAX_EXTENT,
            "difficulty_histogram_u8: a chart of %d x %d (32..%d each way)", H, W, CHART_MAX_EXTENT);
  const ChartGeom g = chart_geom(H, W, bins);
  D3F_CHECK(bins >= 1 && bins <= g.IW, "difficulty_histogram_u8: %d bins outside 1..%d (the box is %d columns wide inside)",
            bins, g.IW, g.IW);
  D3F_CHECK(g.IH >= 1, "difficulty_histogram_u8: a chart of %d rows has no room inside its box", H);
  long long* partial = reinterpret_cast<long long*>(workspace);
  const int nparts = diff_blocks(N);
  hipLaunchKernelGGL(class_minmax_partial_kernel, dim3(nparts), dim3(DIFF_THREADS), 0, stream, classes, N, partial,
                     bin_counts, bins);
  D3F_HIP(hipGetLastError());
  hipLaunchKernelGGL(class_histogram_kernel, dim3(diff_blocks(N)), dim3(DIFF_THREADS), 0, stream, classes, N, bins, partial,
                     nparts, bin_counts, range);
  D3F_HIP(hipGetLastError());
  hipLaunchKernelGGL(histogram_chart_kernel, dim3(cdiv((long)H * W, DIFF_THREADS)), dim3(DIFF_THREADS), 0, stream, g,
                     bin_counts, chart);
  D3F_HIP(hipGetLastError());
  return 0;
}

}  // namespace d3f
