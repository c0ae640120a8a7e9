// Device dataset: training batches assembled on the device from a resident uint8 pool (pointwise.h: pool_batch_launch).
//
// The training set of the reference is the few thousand 448x448 frames of one video, read again every epoch
// (d3f/dataset/image_dataset.py:33-44, decoded on the host, normalised and augmented by the transform of
// d3f/train_deep_fake/lit_module.py:99-111 or the step of d3f/train_denoiser/lit_module.py:55-65,113).  Here the list is
// decoded ONCE into pool [N][H][W][3] uint8 RGB in HBM and one launch per batch does gather + normalise + augmentation:
// 3 bytes read and 12 written per pixel, no image byte over PCIe in steady state.
//
// Memory behaviour: a pool is larger than the 256 MiB Infinity Cache and an image is read once per epoch, so the plain
// path reads it with non-temporal loads (nothing to keep; the weights and activations of the step keep their lines).  The
// warped path reads each texel up to four times from neighbouring lanes and keeps ordinary loads: the re-reads hit L1 / L2.
// The output is consumed by the very next kernel (the noise blend): ordinary stores.
#include "pointwise.h"

namespace d3f {

struct PoolBatchArgs {
  const uint8_t* pool;   // [N][H][W][3]
  const int64_t* index;  // [B]
  float* out;            // [B][3][H][W]
  const float* theta;    // [B][2][3] or null
  const uint8_t* apply;  // [B] or null (theta form: every image warped)
  int64_t N;
  int H, W;
  U8Normalise norm;
  int rng;               // the draws of affine_theta_rng instead of theta / apply
  uint64_t seed, offset;
  AffineRngParams q;
  // balanced sampling (pool_batch_kernel<true> only): the index is drawn too (balanced_index_rng) and written out
  const int64_t* members;      // [M]
  const int64_t* class_start;  // [Kn + 1]
  int64_t* index_out;          // [B]
  int Kn;
};

// One image per blockIdx.y, as affine_warp_rng_kernel: whether the image is warped, passed through or refused is uniform
// per workgroup.  The image's base is a 64-bit pointer (index * H * W * 3 passes 2^32 for ordinary pools); offsets inside
// an image are 32-bit (the host refuses an image of 2^31 bytes or more).  Image bases and rows are not dword-aligned in
// general (5 x 7 x 3 = 105 bytes): the byte path is the general one, the dword path runs where base and size allow it.
// BALANCED: the image's index is not read from a.index but drawn by thread 0 in front of its theta (every workgroup of
// an image draws the same value; workgroup x = 0 stores it to index_out[b]) and handed over through LDS with theta, so the
// range check moves behind the barrier.  The instantiation of the existing entries is the code it was.
template <bool BALANCED>
__global__ __launch_bounds__(256) void pool_batch_kernel(PoolBatchArgs a) {
  __shared__ float th[6];
  __shared__ int warped;
  __shared__ int64_t drawn;
  const int b = blockIdx.y;
  const int HW = a.H * a.W;
  int64_t idx = BALANCED ? 0 : a.index[b];
  float* __restrict__ o = a.out + (size_t)b * 3 * (size_t)HW;
  const int first = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
  const auto outside = [&]() {  // nothing is read for this image
    if (idx >= 0 && idx < a.N) return false;
    const float nan = __builtin_nanf("");
    for (int i = first; i < 3 * HW; i += step) o[i] = nan;
    return true;
  };
  if (!BALANCED && outside()) return;
  if (threadIdx.x == 0) {
    if (BALANCED) {
      const int64_t i = balanced_index_rng(a.seed, a.offset, b, a.members, a.class_start, a.Kn);
      drawn = i;
      if (blockIdx.x == 0) a.index_out[b] = i;
    }
    float t[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int w = 0;
    if (a.rng) {
      w = affine_theta_rng(a.seed, a.offset, b, a.q, t) ? 1 : 0;
    } else if (a.theta != nullptr && (a.apply == nullptr || a.apply[b] != 0)) {
      for (int k = 0; k < 6; ++k) t[k] = a.theta[(long)b * 6 + k];
      w = 1;
    }
    warped = w;
    for (int k = 0; k < 6; ++k) th[k] = t[k];
  }
  __syncthreads();
  if (BALANCED) {
    idx = drawn;
    if (outside()) return;
  }
  const uint8_t* __restrict__ img = a.pool + (size_t)idx * ((size_t)HW * 3);
  if (warped) {
    float t[6];
    for (int k = 0; k < 6; ++k) t[k] = th[k];
    const PoolTexels src{img, a.norm};
    for (int pix = first; pix < HW; pix += step) affine_warp_pixel(src, o, t, pix, 3, a.H, a.W);
    return;
  }
  if ((HW & 3) == 0 && ((uintptr_t)img & 3) == 0 && ((uintptr_t)o & 15) == 0) {
    // four pixels = three dwords in, one float4 per plane out (HW % 4 == 0 keeps every plane 16-byte aligned)
    const uint32_t* __restrict__ words = (const uint32_t*)img;
    for (int g = first; g < HW / 4; g += step) {
      const uint32_t w0 = __builtin_nontemporal_load(words + 3 * g), w1 = __builtin_nontemporal_load(words + 3 * g + 1),
                     w2 = __builtin_nontemporal_load(words + 3 * g + 2);
      const auto byte = [](uint32_t w, int k) { return (uint8_t)(w >> (8 * k)); };
      const float4 r = make_float4(a.norm(byte(w0, 0), 0), a.norm(byte(w0, 3), 0), a.norm(byte(w1, 2), 0),
                                   a.norm(byte(w2, 1), 0));
      const float4 gr = make_float4(a.norm(byte(w0, 1), 1), a.norm(byte(w1, 0), 1), a.norm(byte(w1, 3), 1),
                                    a.norm(byte(w2, 2), 1));
      const float4 bl = make_float4(a.norm(byte(w0, 2), 2), a.norm(byte(w1, 1), 2), a.norm(byte(w2, 0), 2),
                                    a.norm(byte(w2, 3), 2));
      *(float4*)(o + 4 * g) = r;
      *(float4*)(o + HW + 4 * g) = gr;
      *(float4*)(o + 2 * HW + 4 * g) = bl;
    }
    return;
  }
  for (int pix = first; pix < HW; pix += step) {
    const uint8_t* px = img + pix * 3;
    o[pix] = a.norm(__builtin_nontemporal_load(px), 0);
    o[HW + pix] = a.norm(__builtin_nontemporal_load(px + 1), 1);
    o[2 * HW + pix] = a.norm(__builtin_nontemporal_load(px + 2), 2);
  }
}

// `draws written out` twin of the balanced form: the indices alone
__global__ __launch_bounds__(64) void balanced_index_draw_kernel(uint64_t seed, uint64_t offset,
                                                                 const int64_t* __restrict__ members,
                                                                 const int64_t* __restrict__ class_start, int Kn,
                                                                 int64_t* __restrict__ index_out, int B) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b < B) index_out[b] = balanced_index_rng(seed, offset, b, members, class_start, Kn);
}

static int pool_batch_shape_check(int B, int H, int W) {
  const long HW = (long)H * W;
  D3F_CHECK(HW * 3 < (1L << 31), "pool_batch: an image of %ld bytes (H x W x 3 must stay below 2^31)", HW * 3);
  D3F_CHECK(B <= 65535, "pool_batch: B %d above 65535 images per launch", B);
  return 0;
}
static dim3 pool_batch_grid(int B, int H, int W) {
  long bx = ((long)H * W + 255) / 256;
  if (bx > 128) bx = 128;
  return dim3((unsigned)bx, (unsigned)B);
}

int pool_batch_launch(const uint8_t* pool, int64_t N, const int64_t* index, float* out, int B, int H, int W,
                      const float mean[3], const float stdv[3], const float* theta, const uint8_t* apply, uint64_t seed,
                      uint64_t offset, const AffineRngParams* q, hipStream_t stream) {
  if (int rc = pool_batch_shape_check(B, H, W)) return rc;
  if (B == 0) return 0;
  PoolBatchArgs a{};
  a.pool = pool, a.index = index, a.out = out, a.theta = theta, a.apply = apply;
  a.N = N, a.H = H, a.W = W;
  a.norm = U8Normalise{mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2]};
  if (q != nullptr) a.rng = 1, a.seed = seed, a.offset = offset, a.q = *q;
  hipLaunchKernelGGL(pool_batch_kernel<false>, pool_batch_grid(B, H, W), dim3(256), 0, stream, a);
  D3F_HIP(hipGetLastError());
  return 0;
}

int pool_batch_balanced_launch(const uint8_t* pool, int64_t N, const int64_t* members, const int64_t* class_start, int Kn,
                               float* out, int64_t* index_out, int B, int H, int W, const float mean[3],
                               const float stdv[3], uint64_t seed, uint64_t offset, const AffineRngParams* q,
                               hipStream_t stream) {
  if (int rc = pool_batch_shape_check(B, H, W)) return rc;
  if (B == 0) return 0;
  PoolBatchArgs a{};
  a.pool = pool, a.out = out, a.members = members, a.class_start = class_start, a.index_out = index_out, a.Kn = Kn;
  a.N = N, a.H = H, a.W = W;
  a.norm = U8Normalise{mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2]};
  a.seed = seed, a.offset = offset;  // the index draw needs the stream with or without an augmentation
  if (q != nullptr) a.rng = 1, a.q = *q;
  hipLaunchKernelGGL(pool_batch_kernel<true>, pool_batch_grid(B, H, W), dim3(256), 0, stream, a);
  D3F_HIP(hipGetLastError());
  return 0;
}

int balanced_index_draw_launch(const int64_t* members, const int64_t* class_start, int Kn, uint64_t seed, uint64_t offset,
                               int64_t* index_out, int B, hipStream_t stream) {
  D3F_CHECK(B <= 65535, "balanced_index_draw: B %d above 65535 images per launch", B);
  if (B == 0) return 0;
  hipLaunchKernelGGL(balanced_index_draw_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, stream, seed, offset, members,
                     class_start, Kn, index_out, B);
  D3F_HIP(hipGetLastError());
  return 0;
}

}  // namespace d3f
