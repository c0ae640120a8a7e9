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
};

// One image per blockIdx.y, as affine_warp_rng_kernel: whether the image is warped, passed through or refused is uniform
// per workgroup.  The image's base is a 64-bit pointer (index * H * W * 3 passes 2^32 for ordinary pools); offsets inside
// an image are 32-bit (the host refuses an image of 2^31 bytes or more).  Image bases and rows are not dword-aligned in
// general (5 x 7 x 3 = 105 bytes): the byte path is the general one, the dword path runs where base and size allow it.
__global__ __launch_bounds__(256) void pool_batch_kernel(PoolBatchArgs a) {
  __shared__ float th[6];
  __shared__ int warped;
  const int b = blockIdx.y;
  const int HW = a.H * a.W;
  const int64_t idx = a.index[b];
  float* __restrict__ o = a.out + (size_t)b * 3 * (size_t)HW;
  const int first = blockIdx.x * 256 + threadIdx.x, step = gridDim.x * 256;
  if (idx < 0 || idx >= a.N) {  // nothing is read for this image
    const float nan = __builtin_nanf("");
    for (int i = first; i < 3 * HW; i += step) o[i] = nan;
    return;
  }
  if (threadIdx.x == 0) {
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

int pool_batch_launch(const uint8_t* pool, int64_t N, const int64_t* index, float* out, int B, int H, int W,
                      const float mean[3], const float stdv[3], const float* theta, const uint8_t* apply, uint64_t seed,
                      uint64_t offset, const AffineRngParams* q, hipStream_t stream) {
  const long HW = (long)H * W;
  D3F_CHECK(HW * 3 < (1L << 31), "pool_batch: an image of %ld bytes (H x W x 3 must stay below 2^31)", HW * 3);
  D3F_CHECK(B <= 65535, "pool_batch: B %d above 65535 images per launch", B);
  if (B == 0) return 0;
  PoolBatchArgs a{};
  a.pool = pool, a.index = index, a.out = out, a.theta = theta, a.apply = apply;
  a.N = N, a.H = H, a.W = W;
  a.norm = U8Normalise{mean[0], mean[1], mean[2], stdv[0], stdv[1], stdv[2]};
  if (q != nullptr) a.rng = 1, a.seed = seed, a.offset = offset, a.q = *q;
  long bx = (HW + 255) / 256;
  if (bx > 128) bx = 128;
  hipLaunchKernelGGL(pool_batch_kernel, dim3((unsigned)bx, (unsigned)B), dim3(256), 0, stream, a);
  D3F_HIP(hipGetLastError());
  return 0;
}

}  // namespace d3f
