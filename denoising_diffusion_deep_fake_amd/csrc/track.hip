// Template tracker (include/d3f_hip.h: d3f_gray_decimate_u8, d3f_track_seed_u8, d3f_track_search_u8, d3f_track_template_u8): a
// face box marked by hand at a key frame is followed from frame to frame by the smallest sum of absolute differences of a
// reduced grey template.  Everything is integer arithmetic -- exact, and the same in any order of evaluation;
// tests/track_restatement.py restates it in numpy and Python integers.
//
// gray_decimate_kernel (the per-frame hot path: every byte of every frame once): a workgroup takes one row of the reduced
// image and GD_THREADS of its columns, a lane one column.  The s source rows of the tile are staged in LDS, GD rows at a
// time, as the aligned dwords that cover each row's 3 s tx bytes (byte k of a row's span sits at its dword alignment + k, as
// temporal.hip stages its tiles; a dword is loaded whole only inside the frames' bytes, up to GD_ROWS * GD_UNROLL loads of a lane
// in flight), so the global loads are whole dwords at consecutive addresses whatever the byte address of the row.  A lane
// then reads the dwords that cover its 3 s bytes, rotates each pair into place (v_alignbyte_b32) and weights the bytes B G R
// with 1 2 1 by position in the 12-byte group (three dwords are four pixels: three constant weight words, v_dot4_u32_u8); the
// bytes of the last dword past the lane's span are masked.  The sum, at most 4 * 255 * 1024, stays in 32 bits.
//
// track_search_kernel: ONE workgroup for the whole call and the loop over the call's frames inside the kernel, as
// temporal_filter_kernel has it: frame k starts where frame k - 1 ended.  The template lives in LDS for the call (rows 64
// bytes apart, zero behind tw), the position in every lane's registers.  Per frame the clipped search window (at most
// 192 x 192 bytes) is staged as aligned dwords, a row at whatever byte phase its address has; a lane takes four candidates
// next to each other in dx and a part of the template's rows, and walks them a dword at a time -- three of the window's
// dwords rotated into 64 bits at the row's phase, v_qsad_pk_u16_u8 against the template's dword (four sums of absolute
// differences, the window at byte offsets 0..3), the last dword of a row with v_sad_u8 and a mask where tw is no multiple
// of 4; the parts are added and the 64-bit keys reduced with shuffles and through LDS; every lane decodes the winner, the
// lanes blend the template, lane 0 stores the output row.
//
// track_search_scale_kernel (d3f_track_search_scale_u8, opt-in): the same search over the neighbouring sizes too; its own
// comment stands in front of it, tests/track_scale_restatement.py restates it.
//
// track_search_rot_kernel and track_seed_rot_kernel (d3f_track_search_rot_u8, d3f_track_seed_rot_u8, opt-in): the same
// search over the neighbouring angles of the box too, the cost on a disc; their comment stands in front of them,
// tests/track_rot_restatement.py restates them.
//
// track_global_kernel and track_search_reacq_kernel (d3f_track_global_u8, d3f_track_search_reacq_u8, opt-in): the key template
// against every position of the reduced image, over all CUs, and the serial search that takes a frame it does not find from
// there; their comments stand in front of them, tests/track_reacq_restatement.py restates them.  The row walk of all five
// search kernels is one device function, track_row_sad4.
#include "../../include/d3f_hip.h"
#include "common.h"
#include "pointwise.h"

namespace d3f {

typedef unsigned long long u64;

constexpr int TRACK_MAX_SIDE = D3F_TRACK_MAX_SIDE, TRACK_MAX_SEARCH = D3F_TRACK_MAX_SEARCH;
constexpr int TRACK_MAX_STRIDE = D3F_TRACK_MAX_STRIDE, TRACK_MIN_SIDE = 4;
static_assert(TRACK_MAX_SIDE == 64, "the template's LDS rows are 64 bytes; 255 * 64 * 64 < 2^20 is the key's cost field");
static_assert(2 * TRACK_MAX_SEARCH < 256 && 2 * TRACK_MAX_SEARCH * TRACK_MAX_SEARCH < 65536, "the key's fields");

constexpr int GD_THREADS = 256;  // columns of the reduced image a workgroup takes, one per lane
constexpr int GD_UNROLL = 4;     // dwords of a row a lane loads at a time ...
constexpr int GD_ROWS = 4;       // ... of so many rows: 16 loads in flight
constexpr int GD_LDS_DW = 6400;  // staged dwords: one row of the widest tile (s = 32), four of s = 8
static_assert((3 * TRACK_MAX_STRIDE * GD_THREADS + 6) / 4 + 1 <= GD_LDS_DW, "one staged row of the widest tile fits");

// the aligned dword at p: whole where it lies inside [lo, hi), its bytes inside that range otherwise (the rest 0)
__device__ __forceinline__ uint32_t track_load_dword(const uint8_t* p, const uint8_t* lo, const uint8_t* hi) {
  if (p >= lo && p + 4 <= hi) return *reinterpret_cast<const uint32_t*>(p);
  uint32_t v = 0;
  for (int j = 0; j < 4; ++j)
    if (p + j >= lo && p + j < hi) v |= (uint32_t)p[j] << (8 * j);
  return v;
}

struct DecimateGeom {
  int B, h, w, s, gh, gw;
};

__global__ __launch_bounds__(GD_THREADS) void gray_decimate_kernel(const uint8_t* __restrict__ frames, DecimateGeom g,
                                                                  uint8_t* __restrict__ out) {
  __shared__ uint32_t lds[GD_LDS_DW];
  const int tid = threadIdx.x, X0 = blockIdx.x * GD_THREADS, gy = blockIdx.y, b = blockIdx.z;
  const int tx = min(GD_THREADS, g.gw - X0);
  const int span = 3 * g.s * tx;          // bytes of a source row under this tile
  const int row_dw = (span + 6) / 4 + 1;  // up to 3 bytes of alignment in front, and the dword a lane's last rotation reads
  const int R = min(g.s, GD_LDS_DW / row_dw);
  const uint8_t* lo = frames;
  const uint8_t* hi = frames + (long)g.B * g.h * g.w * 3;
  const long pitch = 3L * g.w;
  const uint8_t* seg0 = frames + ((long)b * g.h + (long)gy * g.s) * pitch + 3L * X0 * g.s;
  const int lane_bytes = 3 * g.s, nd = (lane_bytes + 3) / 4;
  uint32_t acc = 0;
  for (int j0 = 0; j0 < g.s; j0 += R) {
    const int rows = min(R, g.s - j0);
    // GD_ROWS rows at a time, so that a lane has GD_ROWS * GD_UNROLL loads in flight before its first LDS store
    for (int r0 = 0; r0 < rows; r0 += GD_ROWS) {
      const uint8_t* first[GD_ROWS];  // row r0 + q: its first aligned dword, and how many hold bytes of the span
      int need[GD_ROWS], need_max = 0;
#pragma unroll
      for (int q = 0; q < GD_ROWS; ++q) {
        const uint8_t* seg = seg0 + (j0 + r0 + q) * pitch;
        const int al = (int)(reinterpret_cast<uintptr_t>(seg) & 3);
        first[q] = seg - al;
        need[q] = r0 + q < rows ? (al + span + 3) / 4 : 0;
        need_max = max(need_max, need[q]);
      }
      for (int k0 = tid; k0 < need_max; k0 += GD_UNROLL * GD_THREADS) {
        uint32_t v[GD_ROWS][GD_UNROLL];
#pragma unroll
        for (int q = 0; q < GD_ROWS; ++q)
#pragma unroll
          for (int u = 0; u < GD_UNROLL; ++u) {
            const int k = k0 + u * GD_THREADS;
            v[q][u] = k < need[q] ? track_load_dword(first[q] + 4 * k, lo, hi) : 0u;
          }
#pragma unroll
        for (int q = 0; q < GD_ROWS; ++q)
#pragma unroll
          for (int u = 0; u < GD_UNROLL; ++u) {
            const int k = k0 + u * GD_THREADS;
            if (k < need[q]) lds[(r0 + q) * row_dw + k] = v[q][u];
          }
      }
    }
    __syncthreads();
    if (tid < tx) {
      for (int r = 0; r < rows; ++r) {
        const int al = (int)(reinterpret_cast<uintptr_t>(seg0 + (j0 + r) * pitch) & 3);
        const int o = al + lane_bytes * tid, ph = o & 3;
        const uint32_t* row = lds + r * row_dw + (o >> 2);
        uint32_t d_lo = row[0];
        int m3 = 0;  // m mod 3: the dword's place in its 12-byte group
        for (int m = 0; m < nd; ++m) {
          const uint32_t d_hi = row[m + 1];
          uint32_t d = __builtin_amdgcn_alignbyte(d_hi, d_lo, ph);
          const int left = lane_bytes - 4 * m;
          if (left < 4) d &= (1u << (8 * left)) - 1u;
          // B G R B | G R B G | R B G R, byte 0 lowest
          const uint32_t weights = m3 == 0 ? 0x01010201u : (m3 == 1 ? 0x02010102u : 0x01020101u);
          acc = __builtin_amdgcn_udot4(d, weights, acc, false);
          m3 = m3 == 2 ? 0 : m3 + 1;
          d_lo = d_hi;
        }
      }
    }
    __syncthreads();
  }
  if (tid < tx) out[((long)b * g.gh + gy) * g.gw + X0 + tid] = (uint8_t)(acc / (uint32_t)(4 * g.s * g.s));
}

// The grey of the key box only: block j is row j of the template, lane i its sample i; T is packed, th rows of tw bytes.
// level > 0: the scale search's state, pos[2] = level (the seed's own, L0).
__global__ __launch_bounds__(64) void track_seed_kernel(const uint8_t* __restrict__ frame, int w, int s, int tx, int ty,
                                                       int tw, int level, uint8_t* __restrict__ templ,
                                                       int* __restrict__ pos) {
  const int i = threadIdx.x, j = blockIdx.x;
  if (j == 0 && i == 0) {
    pos[0] = tx, pos[1] = ty;
    if (level > 0) pos[2] = level;
  }
  if (i >= tw) return;
  const uint8_t* p = frame + ((long)(ty + j) * s * w + (long)(tx + i) * s) * 3;
  uint32_t acc = 0;
  for (int y = 0; y < s; ++y, p += 3L * w)
    for (int x = 0; x < s; ++x) acc += (uint32_t)p[3 * x] + 2u * p[3 * x + 1] + p[3 * x + 2];
  templ[j * tw + i] = (uint8_t)(acc / (uint32_t)(4 * s * s));
}

constexpr int TS_THREADS = 1024;
constexpr int TS_UNROLL = 4;                                  // dword loads a lane has in flight
constexpr int TS_WMAX = TRACK_MAX_SIDE + 2 * TRACK_MAX_SEARCH;  // rows and bytes per row of the widest window
constexpr int TS_STAGE_DW = (TS_WMAX + 3 + 3) / 4;            // dwords that can hold bytes of a window row
constexpr int TS_PITCH_DW = TS_STAGE_DW + 3;                  // and the dwords a lane's last rotation reads behind them
constexpr int TS_TDW = TRACK_MAX_SIDE / 4;                    // dwords of a template row in LDS

struct SearchGeom {
  int B, gh, gw, tw, th, R, adapt, lost;
};

// One row of a template against one staged window row for four candidates next to each other: row, the window row's dword
// that holds the first candidate's first byte, ph that byte's place in it; trow, the template row's dwords (zero behind its
// n bytes); nfull = n >> 2 whole dwords, each three of the window's dwords rotated into 64 bits and one v_qsad_pk_u16_u8
// (four sums of absolute differences, the window at byte offsets 0..3; 16-bit sums: at most 16 dwords of 4 * 255 a row);
// with has_tail (n & 3 != 0) the last, partial dword through v_sad_u8, the window's bytes behind n masked by tail.  The
// four sums are added to cost.  Reads row[0 .. nfull + 1], and row[nfull + 2] with has_tail.
__device__ __forceinline__ void track_row_sad4(const uint32_t* row, int ph, const uint32_t* trow, int nfull, bool has_tail,
                                               uint32_t tail, uint32_t (&cost)[4]) {
  uint32_t d0 = row[0], d1 = row[1];
  u64 acc = 0;
  for (int m = 0; m < nfull; ++m) {
    const uint32_t d2 = row[m + 2];
    const uint32_t w0 = __builtin_amdgcn_alignbyte(d1, d0, ph), w1 = __builtin_amdgcn_alignbyte(d2, d1, ph);
    acc = __builtin_amdgcn_qsad_pk_u16_u8((u64)w1 << 32 | w0, trow[m], acc);
    d0 = d1, d1 = d2;
  }
  if (has_tail) {
    const uint32_t d2 = row[nfull + 2];
    const uint32_t w0 = __builtin_amdgcn_alignbyte(d1, d0, ph), w1 = __builtin_amdgcn_alignbyte(d2, d1, ph);
    const uint32_t t = trow[nfull];
#pragma unroll
    for (int i = 0; i < 4; ++i) cost[i] = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w1, w0, i) & tail, t, cost[i]);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) cost[i] += (uint32_t)(acc >> (16 * i)) & 0xffffu;
}

// The serial search in its two forms.  REACQ false: track_search_kernel, what d3f_track_search_u8 specifies.  REACQ true:
// track_search_reacq_kernel (d3f_track_search_reacq_u8): a frame that the window does not find takes the whole-frame
// search's keys[b] (track_global_kernel, below) -- at a cost of at most relost a sample the position becomes the key's,
// the template the key template's bytes and the row (x, y, gcost, 2); otherwise the frame is lost as in the plain form.
template <bool REACQ>
__device__ __forceinline__ void track_search_body(const uint8_t* __restrict__ gray, const SearchGeom& g,
                                                  uint8_t* __restrict__ templ, int* __restrict__ pos, int* __restrict__ out,
                                                  const uint8_t* __restrict__ key_templ, const u64* __restrict__ keys,
                                                  int relost) {
  __shared__ uint32_t win[TS_WMAX * TS_PITCH_DW];
  __shared__ uint32_t tl[TRACK_MAX_SIDE * TS_TDW];
  __shared__ u64 red[TS_THREADS / 64];
  uint8_t* tb = reinterpret_cast<uint8_t*>(tl);
  const uint8_t* wb = reinterpret_cast<const uint8_t*>(win);
  const int tid = threadIdx.x, tw = g.tw, th = g.th, R = g.R;
  for (int i = tid; i < TRACK_MAX_SIDE * TS_TDW; i += TS_THREADS) tl[i] = 0;
  __syncthreads();
  for (int i = tid; i < tw * th; i += TS_THREADS) tb[(i / tw) * TRACK_MAX_SIDE + i % tw] = templ[i];
  // a position the host never saw: kept inside the image, so that no candidate reads outside it
  int px = min(max(pos[0], 0), g.gw - tw), py = min(max(pos[1], 0), g.gh - th);
  __syncthreads();
  const int nfull = tw >> 2;  // whole dwords of a template row
  const uint32_t tail = (tw & 3) ? (1u << (8 * (tw & 3))) - 1u : 0xffffffffu;
  const uint8_t* lo = gray;
  const uint8_t* hi = gray + (long)g.B * g.gh * g.gw;
  for (int b = 0; b < g.B; ++b) {
    const int dx_lo = max(-R, -px), dx_hi = min(R, g.gw - tw - px);
    const int dy_lo = max(-R, -py), dy_hi = min(R, g.gh - th - py);
    const int ncx = dx_hi - dx_lo + 1, ncy = dy_hi - dy_lo + 1;
    const int wx0 = px + dx_lo, wy0 = py + dy_lo, ww = ncx - 1 + tw, wh = ncy - 1 + th;
    const uint8_t* seg0 = gray + ((long)b * g.gh + wy0) * g.gw + wx0;
    const int a0 = (int)(reinterpret_cast<uintptr_t>(seg0) & 3);  // row r of the window starts (a0 + r gw) mod 4 past a dword
    const int items = wh * TS_STAGE_DW;
    for (int i0 = tid; i0 < items; i0 += TS_UNROLL * TS_THREADS) {
      uint32_t v[TS_UNROLL];
      int at[TS_UNROLL];
#pragma unroll
      for (int u = 0; u < TS_UNROLL; ++u) {
        const int i = i0 + u * TS_THREADS;
        at[u] = -1;
        v[u] = 0;
        if (i >= items) continue;
        const int r = i / TS_STAGE_DW, k = i - r * TS_STAGE_DW;
        const int al = (a0 + r * g.gw) & 3;
        if (4 * k >= al + ww) continue;
        at[u] = r * TS_PITCH_DW + k;
        v[u] = track_load_dword(seg0 + (long)r * g.gw - al + 4 * k, lo, hi);
      }
#pragma unroll
      for (int u = 0; u < TS_UNROLL; ++u)
        if (at[u] >= 0) win[at[u]] = v[u];
    }
    __syncthreads();
    // A work item is four candidates next to each other in dx (one v_qsad_pk_u16_u8 a template dword: the window's 64 bits at
    // four byte offsets) and one of p parts of the template's rows; the p lanes of a group of four lie next to each other
    // and add their partial costs with shuffles.  p, a power of two: whatever leaves the fewest rows to the busiest lane.
    const int ngx = (ncx + 3) >> 2, ngroups = ngx * ncy;
    int p = 1, units = ((ngroups + TS_THREADS - 1) / TS_THREADS) * th;
    for (int q = 2; q <= 64; q <<= 1) {
      const int u = ((ngroups * q + TS_THREADS - 1) / TS_THREADS) * ((th + q - 1) / q);
      if (u < units) p = q, units = u;
    }
    const int rpp = (th + p - 1) / p;
    u64 best = ~0ull;
    for (int it0 = 0; it0 < ngroups * p; it0 += TS_THREADS) {
      const int item = it0 + tid, grp = item / p, part = item - grp * p;
      const bool live = grp < ngroups;
      const int cyr = live ? grp / ngx : 0, cxr = live ? (grp - cyr * ngx) * 4 : 0;
      uint32_t cost[4] = {0, 0, 0, 0};
      if (live) {
        const int j1 = min(th, (part + 1) * rpp);
        for (int j = part * rpp; j < j1; ++j) {
          const int r = cyr + j;
          const int o = ((a0 + r * g.gw) & 3) + cxr, ph = o & 3;
          // (the row's last, partial dword: the window's bytes behind tw masked, the template's are 0)
          track_row_sad4(win + r * TS_PITCH_DW + (o >> 2), ph, tl + j * TS_TDW, nfull, (tw & 3) != 0, tail, cost);
        }
      }
      for (int off = 1; off < p; off <<= 1)
#pragma unroll
        for (int i = 0; i < 4; ++i) cost[i] += __shfl_xor(cost[i], off, 64);
      if (live && part == 0) {
        const int dy = dy_lo + cyr;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int dx = dx_lo + cxr + i;
          if (cxr + i >= ncx) continue;
          const u64 key = (u64)cost[i] << 32 | (u64)(dx * dx + dy * dy) << 16 | (u64)(dy + R) << 8 | (u64)(dx + R);
          best = key < best ? key : best;
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const u64 other = __shfl_xor(best, off, 64);
      best = other < best ? other : best;
    }
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    best = red[0];
    for (int k = 1; k < TS_THREADS / 64; ++k) best = red[k] < best ? red[k] : best;
    const int cost = (int)(best >> 32), dx = (int)(best & 255) - R, dy = (int)((best >> 8) & 255) - R;
    const int found = cost <= g.lost * tw * th;
    int row_cost = cost, row_found = found;  // what the output row says: the whole-frame search may change both
    if (found) {
      px += dx, py += dy;
      if (g.adapt > 0)
        for (int idx = tid; idx < tw * th; idx += TS_THREADS) {
          const int j = idx / tw, i = idx - j * tw, r = py - wy0 + j;
          const int wv = wb[r * (TS_PITCH_DW * 4) + ((a0 + r * g.gw) & 3) + (px - wx0) + i];
          uint8_t* t = tb + j * TRACK_MAX_SIDE + i;
          *t = (uint8_t)((*t * (8 - g.adapt) + wv * g.adapt + 4) >> 3);
        }
    }
    if constexpr (REACQ) {
      if (!found) {
        const u64 gkey = keys[b];  // the same for every lane
        const uint32_t gcost = (uint32_t)(gkey >> 32);
        if (gcost <= (uint32_t)(relost * tw * th)) {
          // (a key the whole-frame search never wrote: kept inside the image, as the position at the start is)
          px = min((int)(gkey & 0xffffu), g.gw - tw), py = min((int)((gkey >> 16) & 0xffffu), g.gh - th);
          for (int idx = tid; idx < tw * th; idx += TS_THREADS) tb[(idx / tw) * TRACK_MAX_SIDE + idx % tw] = key_templ[idx];
          row_cost = (int)gcost, row_found = 2;
        }
      }
    }
    if (tid == 0) {
      int* o = out + 4L * b;
      o[0] = px, o[1] = py, o[2] = row_cost, o[3] = row_found;
    }
    __syncthreads();  // the window, the template and red are the next frame's
  }
  for (int i = tid; i < tw * th; i += TS_THREADS) templ[i] = tb[(i / tw) * TRACK_MAX_SIDE + i % tw];
  if (tid == 0) pos[0] = px, pos[1] = py;
}

__global__ __launch_bounds__(TS_THREADS) void track_search_kernel(const uint8_t* __restrict__ gray, SearchGeom g,
                                                                 uint8_t* __restrict__ templ, int* __restrict__ pos,
                                                                 int* __restrict__ out) {
  track_search_body<false>(gray, g, templ, pos, out, nullptr, nullptr, 0);
}

__global__ __launch_bounds__(TS_THREADS) void track_search_reacq_kernel(const uint8_t* __restrict__ gray, SearchGeom g,
                                                                       uint8_t* __restrict__ templ, int* __restrict__ pos,
                                                                       int* __restrict__ out,
                                                                       const uint8_t* __restrict__ key_templ,
                                                                       const u64* __restrict__ keys, int relost) {
  track_search_body<true>(gray, g, templ, pos, out, key_templ, keys, relost);
}

// ---- the whole-frame search (include/d3f_hip.h: d3f_track_global_u8; tests/track_reacq_restatement.py) ----
// track_global_kernel: the key template K against EVERY position of the reduced image, the frames independent of each other:
// the grid is (tiles of TG_X x TG_Y candidate positions, B), a workgroup of TG_THREADS lanes a tile.  It stages K (rows 64
// bytes apart, zero behind tw) and the (TG_Y - 1 + th) x (TG_X - 1 + tw) window its tile needs as aligned dwords, a row at
// whatever byte phase its address has, as track_search_kernel stages its window; a lane takes four candidates next to each
// other in x and one of TG_PARTS parts of the template's rows (track_row_sad4, the serial search's walk), the parts are
// added with shuffles, the tile's keys cost << 32 | y << 16 | x reduced with shuffles and through LDS, and lane 0 takes the
// minimum into keys[b] with ONE 64-bit atomicMin (a vector atomic, global_atomic_umin_x2) -- on keys that
// track_keys_fill_kernel, the launch before it on the stream, set to all-ones.  A minimum: exact in any order.
// 16 x 8 candidates a tile: a 1080 x 1920 frame at stride 5 (216 x 384, a 48 x 48 template: 337 x 169 candidates) is
// 22 x 22 = 484 tiles, nearly two for each of the 256 CUs at B = 1.  LDS: 71 x 24 dwords of window (6816 bytes), 4096 bytes
// of template and 32 bytes of keys, 10 944 bytes in all.
constexpr int TG_THREADS = 256;
constexpr int TG_X = 16, TG_Y = 8;                            // candidate positions of a tile
constexpr int TG_GROUPS = TG_X / 4 * TG_Y;                    // groups of four candidates
constexpr int TG_PARTS = TG_THREADS / TG_GROUPS;              // lanes of a group, next to each other: parts of the rows
constexpr int TG_WROWS = TG_Y - 1 + TRACK_MAX_SIDE;           // rows and bytes per row of the widest window
constexpr int TG_WBYTES = TG_X - 1 + TRACK_MAX_SIDE;
constexpr int TG_STAGE_DW = (TG_WBYTES + 3 + 3) / 4;          // dwords that can hold bytes of a window row
constexpr int TG_PITCH_DW = TG_STAGE_DW + 3;                  // and the dwords a lane's last rotation reads behind them
static_assert(TG_X % 4 == 0 && TG_GROUPS * TG_PARTS == TG_THREADS && TG_PARTS <= 64 && (TG_PARTS & (TG_PARTS - 1)) == 0,
              "a group's parts are a power of two of neighbouring lanes of one wave");
static_assert((3 + TG_X - 4) / 4 + TRACK_MAX_SIDE / 4 + 1 < TG_PITCH_DW, "the last dword a lane reads lies in its row");

struct GlobalGeom {
  int B, gh, gw, tw, th, ntx;  // ntx: tiles in a row of tiles
};

__global__ __launch_bounds__(256) void track_keys_fill_kernel(u64* __restrict__ keys, int B) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < B) keys[i] = ~0ull;
}

__global__ __launch_bounds__(TG_THREADS) void track_global_kernel(const uint8_t* __restrict__ gray, GlobalGeom g,
                                                                 const uint8_t* __restrict__ key_templ,
                                                                 u64* __restrict__ keys) {
  __shared__ uint32_t win[TG_WROWS * TG_PITCH_DW];
  __shared__ uint32_t tl[TRACK_MAX_SIDE * TS_TDW];
  __shared__ u64 red[TG_THREADS / 64];
  const int tid = threadIdx.x, tw = g.tw, th = g.th, b = blockIdx.y;
  const int tile_y = blockIdx.x / g.ntx, tile_x = blockIdx.x - tile_y * g.ntx;
  const int x0 = tile_x * TG_X, y0 = tile_y * TG_Y;
  const int ncx = min(TG_X, g.gw - tw + 1 - x0), ncy = min(TG_Y, g.gh - th + 1 - y0);  // the tile's candidates: both >= 1
  const int ww = ncx - 1 + tw, wh = ncy - 1 + th;                                      // its window, inside the image
  // K: a lane a dword of a row, the bytes behind tw as 0 (the tail's mask relies on it)
  for (int idx = tid; idx < th * TS_TDW; idx += TG_THREADS) {
    const int j = idx / TS_TDW, m4 = idx - j * TS_TDW;
    uint32_t d = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (4 * m4 + q < tw) d |= (uint32_t)key_templ[j * tw + 4 * m4 + q] << (8 * q);
    tl[idx] = d;
  }
  const uint8_t* lo = gray;
  const uint8_t* hi = gray + (long)g.B * g.gh * g.gw;
  const uint8_t* seg0 = gray + ((long)b * g.gh + y0) * g.gw + x0;
  const int a0 = (int)(reinterpret_cast<uintptr_t>(seg0) & 3);  // row r of the window starts (a0 + r gw) mod 4 past a dword
  const int items = wh * TG_STAGE_DW;
  for (int i0 = tid; i0 < items; i0 += TS_UNROLL * TG_THREADS) {
    uint32_t v[TS_UNROLL];
    int at[TS_UNROLL];
#pragma unroll
    for (int u = 0; u < TS_UNROLL; ++u) {
      const int i = i0 + u * TG_THREADS;
      at[u] = -1;
      v[u] = 0;
      if (i >= items) continue;
      const int r = i / TG_STAGE_DW, k = i - r * TG_STAGE_DW;
      const int al = (a0 + r * g.gw) & 3;
      if (4 * k >= al + ww) continue;
      at[u] = r * TG_PITCH_DW + k;
      v[u] = track_load_dword(seg0 + (long)r * g.gw - al + 4 * k, lo, hi);
    }
#pragma unroll
    for (int u = 0; u < TS_UNROLL; ++u)
      if (at[u] >= 0) win[at[u]] = v[u];
  }
  __syncthreads();
  const int grp = tid / TG_PARTS, part = tid - grp * TG_PARTS;
  const int cyr = grp / (TG_X / 4), cxr = (grp - cyr * (TG_X / 4)) * 4;
  const bool live = cyr < ncy && cxr < ncx;
  const int nfull = tw >> 2;  // whole dwords of a template row
  const uint32_t tail = (tw & 3) ? (1u << (8 * (tw & 3))) - 1u : 0xffffffffu;
  const int rpp = (th + TG_PARTS - 1) / TG_PARTS;
  uint32_t cost[4] = {0, 0, 0, 0};
  if (live) {
    const int j1 = min(th, (part + 1) * rpp);
    for (int j = part * rpp; j < j1; ++j) {
      const int r = cyr + j;
      const int o = ((a0 + r * g.gw) & 3) + cxr, ph = o & 3;
      track_row_sad4(win + r * TG_PITCH_DW + (o >> 2), ph, tl + j * TS_TDW, nfull, (tw & 3) != 0, tail, cost);
    }
  }
#pragma unroll
  for (int off = 1; off < TG_PARTS; off <<= 1)
#pragma unroll
    for (int i = 0; i < 4; ++i) cost[i] += __shfl_xor(cost[i], off, 64);
  u64 best = ~0ull;
  if (live && part == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (cxr + i >= ncx) continue;
      const u64 key = (u64)cost[i] << 32 | (u64)(y0 + cyr) << 16 | (u64)(x0 + cxr + i);
      best = key < best ? key : best;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const u64 other = __shfl_xor(best, off, 64);
    best = other < best ? other : best;
  }
  if ((tid & 63) == 0) red[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    for (int k = 1; k < TG_THREADS / 64; ++k) best = red[k] < best ? red[k] : best;
    atomicMin(keys + b, best);
  }
}

// ---- the scale search (include/d3f_hip.h: d3f_track_search_scale_u8; tests/track_scale_restatement.py) ----
// track_search_scale_kernel keeps the shape of track_search_kernel: ONE workgroup, the loop over the call's frames inside,
// the position and the level in every lane's registers.  The state's template T0 stays at the seed's size tw0 x th0 in LDS
// for the call; per frame it is resampled to the sizes of the (up to three) candidate levels, the union of their search
// windows is staged once as aligned dwords, and the candidates of all levels are spread over the lanes as work items of
// four dx and a part of the rows, as above.  A key-writing lane divides once per candidate (the cost over the area); the
// winner's window is resampled back to the seed's size and blended into T0.
constexpr int SS_LEVELS = 3;                                          // dL = -1, 0, 1
constexpr int SS_WMAX = TRACK_MAX_SIDE + 2 * TRACK_MAX_SEARCH + 2;    // the union window: anchors of neighbouring levels lie
constexpr int SS_STAGE_DW = (SS_WMAX + 3 + 3) / 4;                    // at most one sample apart, their sizes too
constexpr int SS_PITCH_DW = SS_STAGE_DW + 3;
// a level's entry: valid, tw, th, x and y of its first candidate in the image, dx_lo, dy_lo, ncx, ncy, ngx, anchor x, anchor y
constexpr int SS_LV = 12;
static_assert((SS_WMAX * SS_PITCH_DW + (1 + SS_LEVELS) * TRACK_MAX_SIDE * TS_TDW + SS_LEVELS * 2 * TRACK_MAX_SIDE) * 4 +
                      SS_LEVELS * SS_LV * 4 + TS_THREADS / 64 * 8 <= 64 * 1024,
              "track_search_scale_kernel's static LDS");

struct ScaleGeom {
  int B, gh, gw, tw0, th0, R, adapt, lost, levels, penalty, Lmin, Lmax;  // Lmin..Lmax: the valid levels, found on the host
};

__host__ __device__ __forceinline__ int track_level_side(int n0, int L, int L0) { return (n0 * L + (L0 >> 1)) / L0; }

// the two taps and the 6-bit weight of output sample i of n_out from n_in, bilinear at pixel centres: i0 | i1 << 8 | f << 16
__device__ __forceinline__ uint32_t track_resample_tap(int i, int n_in, int n_out) {
  const int num = (2 * i + 1) * n_in - n_out, den = 2 * n_out;
  int i0 = 0, f = 0;
  if (num >= 0) {
    i0 = num / den;
    f = ((num - i0 * den) * 64) / den;
  }
  const int i1 = min(i0 + 1, n_in - 1);
  i0 = min(i0, n_in - 1);
  return (uint32_t)i0 | (uint32_t)i1 << 8 | (uint32_t)f << 16;
}

__device__ __forceinline__ int track_bilinear(int a00, int a01, int a10, int a11, int fx, int fy) {
  return (a00 * (64 - fy) * (64 - fx) + a01 * (64 - fy) * fx + a10 * fy * (64 - fx) + a11 * fy * fx + 2048) >> 12;
}

__global__ __launch_bounds__(TS_THREADS) void track_search_scale_kernel(const uint8_t* __restrict__ gray, ScaleGeom g,
                                                                       uint8_t* __restrict__ templ, int* __restrict__ pos,
                                                                       int* __restrict__ out) {
  __shared__ uint32_t win[SS_WMAX * SS_PITCH_DW];
  __shared__ uint32_t t0[TRACK_MAX_SIDE * TS_TDW];              // T0, rows 64 bytes apart
  __shared__ uint32_t tl[SS_LEVELS * TRACK_MAX_SIDE * TS_TDW];  // T(Lc) per level, rows 64 bytes apart, zero behind tw(Lc)
  __shared__ uint32_t taps[SS_LEVELS * 2 * TRACK_MAX_SIDE];     // level k: 64 taps in x, then 64 in y
  __shared__ int lv[SS_LEVELS][SS_LV];
  __shared__ u64 red[TS_THREADS / 64];
  uint8_t* t0b = reinterpret_cast<uint8_t*>(t0);
  uint8_t* tlb = reinterpret_cast<uint8_t*>(tl);
  const uint8_t* wb = reinterpret_cast<const uint8_t*>(win);
  const int tid = threadIdx.x, tw0 = g.tw0, th0 = g.th0, R = g.R, L0 = max(tw0, th0);
  for (int i = tid; i < tw0 * th0; i += TS_THREADS) t0b[(i / tw0) * TRACK_MAX_SIDE + i % tw0] = templ[i];
  // a level or a position the host never saw: kept valid, so that no candidate reads outside the image
  int L = min(max(pos[2], g.Lmin), g.Lmax);
  int tw = track_level_side(tw0, L, L0), th = track_level_side(th0, L, L0);
  int px = min(max(pos[0], 0), g.gw - tw), py = min(max(pos[1], 0), g.gh - th);
  const uint8_t* lo = gray;
  const uint8_t* hi = gray + (long)g.B * g.gh * g.gw;
  __syncthreads();
  for (int b = 0; b < g.B; ++b) {
    // each level's entry (one lane) and the taps of T0 -> T(Lc) (a lane a tap)
    if (tid < SS_LEVELS * 2 * TRACK_MAX_SIDE) {
      const int k = tid >> 7, axis = (tid >> 6) & 1, i = tid & 63, Lc = L + k - 1;
      const bool valid = abs(k - 1) <= g.levels && Lc >= g.Lmin && Lc <= g.Lmax;
      const int twc = valid ? track_level_side(tw0, Lc, L0) : 0, thc = valid ? track_level_side(th0, Lc, L0) : 0;
      if (valid && i < (axis ? thc : twc)) taps[tid] = axis ? track_resample_tap(i, th0, thc) : track_resample_tap(i, tw0, twc);
      if ((tid & 127) == 0) {
        int* e = lv[k];
        const int ax = valid ? min(max(px + ((tw - twc) >> 1), 0), g.gw - twc) : 0;  // (>> 1 of a negative: the floor)
        const int ay = valid ? min(max(py + ((th - thc) >> 1), 0), g.gh - thc) : 0;
        const int dx_lo = max(-R, -ax), dx_hi = min(R, g.gw - twc - ax);
        const int dy_lo = max(-R, -ay), dy_hi = min(R, g.gh - thc - ay);
        e[0] = valid, e[1] = twc, e[2] = thc, e[3] = ax + dx_lo, e[4] = ay + dy_lo, e[5] = dx_lo, e[6] = dy_lo;
        e[7] = valid ? dx_hi - dx_lo + 1 : 0, e[8] = valid ? dy_hi - dy_lo + 1 : 0, e[9] = (e[7] + 3) >> 2;
        e[10] = ax, e[11] = ay;
      }
    }
    __syncthreads();
    // the union of the levels' windows, and where each level's groups start among all of them
    int wx0 = g.gw, wy0 = g.gh, wx1 = 0, wy1 = 0, gfirst[SS_LEVELS + 1], thmax = 0;
    gfirst[0] = 0;
#pragma unroll
    for (int k = 0; k < SS_LEVELS; ++k) {
      const int* e = lv[k];
      gfirst[k + 1] = gfirst[k] + e[9] * e[8];
      if (!e[0]) continue;
      wx0 = min(wx0, e[3]), wy0 = min(wy0, e[4]);
      wx1 = max(wx1, e[3] + e[7] - 1 + e[1]), wy1 = max(wy1, e[4] + e[8] - 1 + e[2]);
      thmax = max(thmax, e[2]);
    }
    const int ngroups = gfirst[SS_LEVELS];
    const int ww = min(wx1 - wx0, SS_WMAX), wh = min(wy1 - wy0, SS_WMAX);  // (never above it: see SS_WMAX)
    const uint8_t* seg0 = gray + ((long)b * g.gh + wy0) * g.gw + wx0;
    const int a0 = (int)(reinterpret_cast<uintptr_t>(seg0) & 3);  // row r of the window starts (a0 + r gw) mod 4 past a dword
    const int items = wh * SS_STAGE_DW;
    for (int i0 = tid; i0 < items; i0 += TS_UNROLL * TS_THREADS) {
      uint32_t v[TS_UNROLL];
      int at[TS_UNROLL];
#pragma unroll
      for (int u = 0; u < TS_UNROLL; ++u) {
        const int i = i0 + u * TS_THREADS;
        at[u] = -1;
        v[u] = 0;
        if (i >= items) continue;
        const int r = i / SS_STAGE_DW, k = i - r * SS_STAGE_DW;
        const int al = (a0 + r * g.gw) & 3;
        if (4 * k >= al + ww) continue;
        at[u] = r * SS_PITCH_DW + k;
        v[u] = track_load_dword(seg0 + (long)r * g.gw - al + 4 * k, lo, hi);
      }
#pragma unroll
      for (int u = 0; u < TS_UNROLL; ++u)
        if (at[u] >= 0) win[at[u]] = v[u];
    }
    // T(Lc) = resample(T0): whole dwords of a row are written, the bytes behind tw(Lc) as 0 (the tail's mask relies on it)
#pragma unroll
    for (int k = 0; k < SS_LEVELS; ++k) {
      const int* e = lv[k];
      if (!e[0]) continue;
      const int twc = e[1], thc = e[2], tw4 = (twc + 3) & ~3;
      for (int idx = tid; idx < tw4 * thc; idx += TS_THREADS) {
        const int j = idx / tw4, i = idx - j * tw4;
        int v = 0;
        if (i < twc) {
          const uint32_t tx = taps[k * 128 + i], ty = taps[k * 128 + 64 + j];
          const uint8_t* r0 = t0b + (ty & 255) * TRACK_MAX_SIDE;
          const uint8_t* r1 = t0b + ((ty >> 8) & 255) * TRACK_MAX_SIDE;
          const int x0 = tx & 255, x1 = (tx >> 8) & 255;
          v = track_bilinear(r0[x0], r0[x1], r1[x0], r1[x1], (int)(tx >> 16), (int)(ty >> 16));
        }
        tlb[(k * TRACK_MAX_SIDE + j) * TRACK_MAX_SIDE + i] = (uint8_t)v;
      }
    }
    __syncthreads();
    // work items as in track_search_kernel, over the groups of all levels; p on their sum and the tallest template
    int p = 1, units = ((ngroups + TS_THREADS - 1) / TS_THREADS) * thmax;
    for (int q = 2; q <= 64; q <<= 1) {
      const int u = ((ngroups * q + TS_THREADS - 1) / TS_THREADS) * ((thmax + q - 1) / q);
      if (u < units) p = q, units = u;
    }
    u64 best = ~0ull;
    for (int it0 = 0; it0 < ngroups * p; it0 += TS_THREADS) {
      const int item = it0 + tid, grp = item / p, part = item - grp * p;
      const bool live = grp < ngroups;
      const int k = !live || grp < gfirst[1] ? 0 : (grp < gfirst[2] ? 1 : 2);
      const int* e = lv[k];
      const int twc = e[1], thc = e[2], ncx = e[7], ngx = e[9];
      const int local = live ? grp - (k == 0 ? 0 : (k == 1 ? gfirst[1] : gfirst[2])) : 0;
      const int cyr = live ? local / ngx : 0, cxr = live ? (local - cyr * ngx) * 4 : 0;
      const int nfull = twc >> 2;
      const uint32_t tail = (1u << (8 * (twc & 3))) - 1u;
      uint32_t cost[4] = {0, 0, 0, 0};
      if (live) {
        const int rpp = (thc + p - 1) / p, j1 = min(thc, (part + 1) * rpp);
        const int xo = e[3] - wx0 + cxr, yo = e[4] - wy0 + cyr;
        for (int j = part * rpp; j < j1; ++j) {
          const int r = yo + j;
          const int o = ((a0 + r * g.gw) & 3) + xo, ph = o & 3;
          // (the row's last, partial dword: the window's bytes behind tw(Lc) masked, the template's are 0)
          track_row_sad4(win + r * SS_PITCH_DW + (o >> 2), ph, tl + (k * TRACK_MAX_SIDE + j) * TS_TDW, nfull, (twc & 3) != 0, tail,
                         cost);
        }
      }
      for (int off = 1; off < p; off <<= 1)
#pragma unroll
        for (int i = 0; i < 4; ++i) cost[i] += __shfl_xor(cost[i], off, 64);
      if (live && part == 0) {
        const int dy = e[6] + cyr, adl = k != 1;
        const uint32_t area = (uint32_t)(twc * thc), bias = adl ? (uint32_t)g.penalty : 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int dx = e[5] + cxr + i;
          if (cxr + i >= ncx) continue;
          const uint32_t ncost = (cost[i] << 12) / area;  // cost << 12 <= 255 * 4096 * 4096 < 2^32
          const u64 key = (u64)(ncost + bias) << 33 | (u64)adl << 32 | (u64)k << 30 | (u64)(dx * dx + dy * dy) << 16 |
                          (u64)(dy + R) << 8 | (u64)(dx + R);
          best = key < best ? key : best;
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const u64 other = __shfl_xor(best, off, 64);
      best = other < best ? other : best;
    }
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    best = red[0];
    for (int k = 1; k < TS_THREADS / 64; ++k) best = red[k] < best ? red[k] : best;
    // the winner: its level, its displacement, and its cost back from cost << 12 over the area (the area is at most 4096, so
    // one multiple of 4096 lies in ncost * area .. ncost * area + area - 1)
    const int kb = (int)((best >> 30) & 3), dx = (int)(best & 255) - R, dy = (int)((best >> 8) & 255) - R;
    const int twb = lv[kb][1], thb = lv[kb][2];
    const uint32_t areab = (uint32_t)(twb * thb);
    const uint32_t ncost = (uint32_t)(best >> 33) - (kb != 1 ? (uint32_t)g.penalty : 0u);
    const int cost = (int)((ncost * areab + 4095u) >> 12);
    const int found = cost <= g.lost * (int)areab;
    if (found) {
      L += kb - 1, tw = twb, th = thb;
      px = lv[kb][10] + dx, py = lv[kb][11] + dy;
      // the taps of the window at the new box -> the seed's size
      if (g.adapt > 0 && tid < 2 * TRACK_MAX_SIDE) {
        const int axis = tid >> 6, i = tid & 63;
        if (i < (axis ? th0 : tw0)) taps[tid] = axis ? track_resample_tap(i, th, th0) : track_resample_tap(i, tw, tw0);
      }
    }
    __syncthreads();
    if (found && g.adapt > 0)
      for (int idx = tid; idx < tw0 * th0; idx += TS_THREADS) {
        const int j = idx / tw0, i = idx - j * tw0;
        const uint32_t tx = taps[i], ty = taps[64 + j];
        const int ra = py - wy0 + (int)(ty & 255), rb = py - wy0 + (int)((ty >> 8) & 255);
        const uint8_t* r0 = wb + ra * (SS_PITCH_DW * 4) + ((a0 + ra * g.gw) & 3) + (px - wx0);
        const uint8_t* r1 = wb + rb * (SS_PITCH_DW * 4) + ((a0 + rb * g.gw) & 3) + (px - wx0);
        const int x0 = tx & 255, x1 = (tx >> 8) & 255;
        const int wv = track_bilinear(r0[x0], r0[x1], r1[x0], r1[x1], (int)(tx >> 16), (int)(ty >> 16));
        uint8_t* t = t0b + j * TRACK_MAX_SIDE + i;
        *t = (uint8_t)((*t * (8 - g.adapt) + wv * g.adapt + 4) >> 3);
      }
    if (tid == 0) {
      int* o = out + 8L * b;
      o[0] = px, o[1] = py, o[2] = tw, o[3] = th, o[4] = (int)ncost, o[5] = found, o[6] = L, o[7] = cost;
    }
    __syncthreads();  // the window, the templates, the taps, the levels' entries and red are the next frame's
  }
  for (int i = tid; i < tw0 * th0; i += TS_THREADS) templ[i] = t0b[(i / tw0) * TRACK_MAX_SIDE + i % tw0];
  if (tid == 0) pos[0] = px, pos[1] = py, pos[2] = L;
}

// ---- the rotation search (include/d3f_hip.h: d3f_track_search_rot_u8; tests/track_rot_restatement.py) ----
// track_search_rot_kernel keeps the shape of track_search_kernel: ONE workgroup, the loop over the call's frames inside,
// the position and the angle index uniform for the workgroup (read back from the reduced key through readfirstlane, so
// they stay in scalar registers).  The state's template T0 is the upright face, tw0 x th0, in LDS for the call; the cost is
// taken on the disc of diameter min(tw0, th0) about the box's centre, which a rotation maps onto itself, every row of it one
// span (lo, n).  Per frame T0 is turned to the (up to three) candidate angles -- row j of a turned template holds the
// span's n(j) samples left-aligned, zero behind them, rows RS_TPITCH_DW dwords apart: the odd pitch puts the rows that the
// parts of a group read at once on different banks -- the window is staged as track_search_kernel stages it (the
// candidates' boxes are the un-rotated ones, the same for every angle), and the candidates of all angles are spread over
// the lanes as work items of four dx and a part of the rows.  A row's walk starts lo(j) bytes into the window's row and
// takes n(j) >> 2 whole dwords and a masked tail.  The winner's window is turned back and blended into T0 on the disc.
// The rotations arrive as a table of (c16, s16) per angle index BY VALUE in the kernel's arguments (the host has checked
// every entry; the device does no trigonometry) and are copied to LDS once, where a lane indexes them.
constexpr int RS_ANGLES = 3;                             // dA = -1, 0, 1
constexpr int RS_MAX_INDEX = D3F_TRACK_ROT_MAX_INDEX;    // the angle indices are -amax..amax, amax at most this
constexpr int RS_TABLE = 2 * RS_MAX_INDEX + 1;
constexpr int RS_TPITCH_DW = TS_TDW + 1;                 // dwords between the rows of a turned template
static_assert((TS_WMAX * TS_PITCH_DW + TRACK_MAX_SIDE * TS_TDW + RS_ANGLES * TRACK_MAX_SIDE * RS_TPITCH_DW + TRACK_MAX_SIDE +
               2 * RS_TABLE) * 4 + TS_THREADS / 64 * 8 <= 64 * 1024,
              "track_search_rot_kernel's static LDS");
static_assert(RS_MAX_INDEX < 128 && TRACK_MAX_SIDE <= 64, "the angle index is a byte of the key's decode; a span is lo | n << 8");

struct RotGeom {
  int B, gh, gw, tw0, th0, R, adapt, lost, steps, penalty, amax;
  FrameRot rot[RS_TABLE];  // index a + amax: the rotation by a * step
};

// the disc: sample (i, j) of tw0 x th0 belongs when u u + v v <= D D, u = 2 i + 1 - tw0, v = 2 j + 1 - th0, D = min(tw0, th0)
__device__ __forceinline__ bool track_disc(int i, int j, int tw0, int th0) {
  const int u = 2 * i + 1 - tw0, v = 2 * j + 1 - th0, D = min(tw0, th0);
  return u * u + v * v <= D * D;
}

// Output sample (i, j) of rot(A, c, s): the position in A turned about the centre, in 1/131072 of a sample (below 2^24 in
// magnitude: |u|, |v| < 64, |c|, |s| <= 65536), its two taps per axis clamped to the array and the 6-bit weights
struct RotTap {
  int x0, x1, y0, y1, fx, fy;
};
__device__ __forceinline__ RotTap track_rot_tap(int i, int j, int tw0, int th0, int c, int s) {
  const int u = 2 * i + 1 - tw0, v = 2 * j + 1 - th0;
  const int X = c * u + s * v + (tw0 - 1) * 65536, Y = -s * u + c * v + (th0 - 1) * 65536;
  const int x0 = X >> 17, y0 = Y >> 17;
  return RotTap{min(max(x0, 0), tw0 - 1), min(max(x0 + 1, 0), tw0 - 1), min(max(y0, 0), th0 - 1), min(max(y0 + 1, 0), th0 - 1),
                (X >> 11) & 63,          (Y >> 11) & 63};
}

// The seed with an angle: templ holds the grey of the axis-aligned key box (track_seed_kernel); on the disc it becomes that
// grey turned back by the key angle, rot(grey, c, -s), and pos[2] the angle's index.  One workgroup: every read through LDS
// before the first write.
__global__ __launch_bounds__(TS_THREADS) void track_seed_rot_kernel(uint8_t* __restrict__ templ, int tw0, int th0, int a0, int c,
                                                                   int s, int* __restrict__ pos) {
  __shared__ uint8_t src[TRACK_MAX_SIDE * TRACK_MAX_SIDE];
  const int tid = threadIdx.x;
  for (int idx = tid; idx < tw0 * th0; idx += TS_THREADS) src[idx] = templ[idx];
  if (tid == 0) pos[2] = a0;
  __syncthreads();
  for (int idx = tid; idx < tw0 * th0; idx += TS_THREADS) {
    const int j = idx / tw0, i = idx - j * tw0;
    if (!track_disc(i, j, tw0, th0)) continue;
    const RotTap t = track_rot_tap(i, j, tw0, th0, c, -s);
    const uint8_t* r0 = src + t.y0 * tw0;
    const uint8_t* r1 = src + t.y1 * tw0;
    templ[idx] = (uint8_t)track_bilinear(r0[t.x0], r0[t.x1], r1[t.x0], r1[t.x1], t.fx, t.fy);
  }
}

__global__ __launch_bounds__(TS_THREADS) void track_search_rot_kernel(const uint8_t* __restrict__ gray, RotGeom g,
                                                                     uint8_t* __restrict__ templ, int* __restrict__ pos,
                                                                     int* __restrict__ out) {
  __shared__ uint32_t win[TS_WMAX * TS_PITCH_DW];
  __shared__ uint32_t t0[TRACK_MAX_SIDE * TS_TDW];                     // T0, rows 64 bytes apart
  __shared__ uint32_t tl[RS_ANGLES * TRACK_MAX_SIDE * RS_TPITCH_DW];  // T(a + dA): a row's span left-aligned, zero behind it
  __shared__ uint32_t span[TRACK_MAX_SIDE];                            // row j of the disc: lo | n << 8
  __shared__ int tab[2 * RS_TABLE];                                    // (c16, s16) of index a at 2 (a + amax)
  __shared__ u64 red[TS_THREADS / 64];
  uint8_t* t0b = reinterpret_cast<uint8_t*>(t0);
  const uint8_t* wb = reinterpret_cast<const uint8_t*>(win);
  const int tid = threadIdx.x, tw0 = g.tw0, th0 = g.th0, R = g.R, amax = g.amax;
  for (int i = tid; i < tw0 * th0; i += TS_THREADS) t0b[(i / tw0) * TRACK_MAX_SIDE + i % tw0] = templ[i];
  if (tid < 2 * (2 * amax + 1)) tab[tid] = reinterpret_cast<const int*>(g.rot)[tid];
  if (tid < th0) {
    int lo = 0;
    while (lo < tw0 && !track_disc(lo, tid, tw0, th0)) ++lo;
    span[tid] = lo < tw0 ? (uint32_t)lo | (uint32_t)(tw0 - 2 * lo) << 8 : 0u;  // (the disc is symmetric in i)
  }
  // an angle or a position the host never saw: kept valid, so that no candidate reads outside the table or the image
  int a = __builtin_amdgcn_readfirstlane(min(max(pos[2], -amax), amax));
  int px = __builtin_amdgcn_readfirstlane(min(max(pos[0], 0), g.gw - tw0));
  int py = __builtin_amdgcn_readfirstlane(min(max(pos[1], 0), g.gh - th0));
  const uint8_t* lo = gray;
  const uint8_t* hi = gray + (long)g.B * g.gh * g.gw;
  __syncthreads();
  int n = 0;  // the disc's samples
  for (int j = 0; j < th0; ++j) n += (int)(span[j] >> 8);
  for (int b = 0; b < g.B; ++b) {
    const int dx_lo = max(-R, -px), dx_hi = min(R, g.gw - tw0 - px);
    const int dy_lo = max(-R, -py), dy_hi = min(R, g.gh - th0 - py);
    const int ncx = dx_hi - dx_lo + 1, ncy = dy_hi - dy_lo + 1;
    const int wx0 = px + dx_lo, wy0 = py + dy_lo, ww = ncx - 1 + tw0, wh = ncy - 1 + th0;
    const uint8_t* seg0 = gray + ((long)b * g.gh + wy0) * g.gw + wx0;
    const int a0 = (int)(reinterpret_cast<uintptr_t>(seg0) & 3);  // row r of the window starts (a0 + r gw) mod 4 past a dword
    const int items = wh * TS_STAGE_DW;
    for (int i0 = tid; i0 < items; i0 += TS_UNROLL * TS_THREADS) {
      uint32_t v[TS_UNROLL];
      int at[TS_UNROLL];
#pragma unroll
      for (int u = 0; u < TS_UNROLL; ++u) {
        const int i = i0 + u * TS_THREADS;
        at[u] = -1;
        v[u] = 0;
        if (i >= items) continue;
        const int r = i / TS_STAGE_DW, k = i - r * TS_STAGE_DW;
        const int al = (a0 + r * g.gw) & 3;
        if (4 * k >= al + ww) continue;
        at[u] = r * TS_PITCH_DW + k;
        v[u] = track_load_dword(seg0 + (long)r * g.gw - al + 4 * k, lo, hi);
      }
#pragma unroll
      for (int u = 0; u < TS_UNROLL; ++u)
        if (at[u] >= 0) win[at[u]] = v[u];
    }
    // the candidate angles: k = dA + 1 for a + dA inside the table, always a run kfirst .. kfirst + nk - 1 around k = 1
    const int kfirst = g.steps > 0 && a - 1 >= -amax ? 0 : 1, nk = 2 - kfirst + (g.steps > 0 && a + 1 <= amax ? 1 : 0);
    // T(a + dA) = rot(T0): a lane a dword of a row's span, the bytes behind n(j) as 0 (the tail's mask relies on it)
    for (int idx = tid; idx < nk * th0 * TS_TDW; idx += TS_THREADS) {
      const int kk = idx / (th0 * TS_TDW), rest = idx - kk * (th0 * TS_TDW), j = rest / TS_TDW, m4 = rest - j * TS_TDW;
      const int k = kfirst + kk, lo_j = (int)(span[j] & 255u), n_j = (int)(span[j] >> 8);
      if (4 * m4 >= n_j) continue;
      const int c = tab[2 * (a + k - 1 + amax)], s = tab[2 * (a + k - 1 + amax) + 1];
      uint32_t d = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        if (4 * m4 + q >= n_j) continue;
        const RotTap t = track_rot_tap(lo_j + 4 * m4 + q, j, tw0, th0, c, s);
        const uint8_t* r0 = t0b + t.y0 * TRACK_MAX_SIDE;
        const uint8_t* r1 = t0b + t.y1 * TRACK_MAX_SIDE;
        d |= (uint32_t)track_bilinear(r0[t.x0], r0[t.x1], r1[t.x0], r1[t.x1], t.fx, t.fy) << (8 * q);
      }
      tl[(k * TRACK_MAX_SIDE + j) * RS_TPITCH_DW + m4] = d;
    }
    __syncthreads();
    // work items as in track_search_kernel, over the groups of all angles
    const int ngx = (ncx + 3) >> 2, per = ngx * ncy, ngroups = nk * per;
    int p = 1, units = ((ngroups + TS_THREADS - 1) / TS_THREADS) * th0;
    for (int q = 2; q <= 64; q <<= 1) {
      const int u = ((ngroups * q + TS_THREADS - 1) / TS_THREADS) * ((th0 + q - 1) / q);
      if (u < units) p = q, units = u;
    }
    const int rpp = (th0 + p - 1) / p;
    u64 best = ~0ull;
    for (int it0 = 0; it0 < ngroups * p; it0 += TS_THREADS) {
      const int item = it0 + tid, grp = item / p, part = item - grp * p;
      const bool live = grp < ngroups;
      const int kk = live ? grp / per : 0, local = live ? grp - kk * per : 0, k = kfirst + kk;
      const int cyr = local / ngx, cxr = (local - cyr * ngx) * 4;
      uint32_t cost[4] = {0, 0, 0, 0};
      if (live) {
        const int j1 = min(th0, (part + 1) * rpp);
        for (int j = part * rpp; j < j1; ++j) {
          const int lo_j = (int)(span[j] & 255u), n_j = (int)(span[j] >> 8), nfull = n_j >> 2;
          const int r = cyr + j;
          const int o = ((a0 + r * g.gw) & 3) + cxr + lo_j, ph = o & 3;
          // (the span's last, partial dword: the window's bytes behind n(j) masked, the template's are 0)
          track_row_sad4(win + r * TS_PITCH_DW + (o >> 2), ph, tl + (k * TRACK_MAX_SIDE + j) * RS_TPITCH_DW, nfull, (n_j & 3) != 0,
                         (1u << (8 * (n_j & 3))) - 1u, cost);
        }
      }
      for (int off = 1; off < p; off <<= 1)
#pragma unroll
        for (int i = 0; i < 4; ++i) cost[i] += __shfl_xor(cost[i], off, 64);
      if (live && part == 0) {
        const int dy = dy_lo + cyr, ada = k != 1;
        const uint32_t bias = ada ? (uint32_t)g.penalty : 0u;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int dx = dx_lo + cxr + i;
          if (cxr + i >= ncx) continue;
          const uint32_t ncost = (cost[i] << 12) / (uint32_t)n;  // cost << 12 <= 255 * 4096 * 4096 < 2^32
          const u64 key = (u64)(ncost + bias) << 33 | (u64)ada << 32 | (u64)k << 30 | (u64)(dx * dx + dy * dy) << 16 |
                          (u64)(dy + R) << 8 | (u64)(dx + R);
          best = key < best ? key : best;
        }
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const u64 other = __shfl_xor(best, off, 64);
      best = other < best ? other : best;
    }
    if ((tid & 63) == 0) red[tid >> 6] = best;
    __syncthreads();
    best = red[0];
    for (int k = 1; k < TS_THREADS / 64; ++k) best = red[k] < best ? red[k] : best;
    const uint32_t best_lo = __builtin_amdgcn_readfirstlane((uint32_t)best), best_hi = __builtin_amdgcn_readfirstlane((uint32_t)(best >> 32));
    // the winner: its angle, its displacement, and its cost back from cost << 12 over n (n is at most 4096, so one multiple
    // of 4096 lies in ncost * n .. ncost * n + n - 1)
    const int kb = (int)((best_lo >> 30) & 3u), dx = (int)(best_lo & 255u) - R, dy = (int)((best_lo >> 8) & 255u) - R;
    const uint32_t ncost = (best_hi >> 1) - (kb != 1 ? (uint32_t)g.penalty : 0u);
    const int cost = (int)((ncost * (uint32_t)n + 4095u) >> 12);
    const int found = cost <= g.lost * n;
    if (found) {
      a += kb - 1, px += dx, py += dy;
      if (g.adapt > 0) {
        // W0 = the window at the new box turned back, blended into T0 on the disc
        const int c = tab[2 * (a + amax)], s = -tab[2 * (a + amax) + 1];
        for (int idx = tid; idx < th0 * TRACK_MAX_SIDE; idx += TS_THREADS) {
          const int j = idx >> 6, m = idx & 63, lo_j = (int)(span[j] & 255u), n_j = (int)(span[j] >> 8);
          if (m >= n_j) continue;
          const int i = lo_j + m;
          const RotTap t = track_rot_tap(i, j, tw0, th0, c, s);
          const int ra = py - wy0 + t.y0, rb = py - wy0 + t.y1;
          const uint8_t* r0 = wb + ra * (TS_PITCH_DW * 4) + ((a0 + ra * g.gw) & 3) + (px - wx0);
          const uint8_t* r1 = wb + rb * (TS_PITCH_DW * 4) + ((a0 + rb * g.gw) & 3) + (px - wx0);
          const int wv = track_bilinear(r0[t.x0], r0[t.x1], r1[t.x0], r1[t.x1], t.fx, t.fy);
          uint8_t* tp = t0b + j * TRACK_MAX_SIDE + i;
          *tp = (uint8_t)((*tp * (8 - g.adapt) + wv * g.adapt + 4) >> 3);
        }
      }
    }
    if (tid == 0) {
      int* o = out + 8L * b;
      o[0] = px, o[1] = py, o[2] = tw0, o[3] = th0, o[4] = (int)ncost, o[5] = found, o[6] = a, o[7] = cost;
    }
    __syncthreads();  // the window, the templates and red are the next frame's
  }
  for (int i = tid; i < tw0 * th0; i += TS_THREADS) templ[i] = t0b[(i / tw0) * TRACK_MAX_SIDE + i % tw0];
  if (tid == 0) pos[0] = px, pos[1] = py, pos[2] = a;
}

static int track_frame_check(const char* who, int h, int w, int s) {
  D3F_CHECK(h > 0 && w > 0 && h <= 16384 && w <= 16384, "%s: size %d x %d outside 1..16384", who, h, w);
  D3F_CHECK(s >= 1 && s <= TRACK_MAX_STRIDE, "%s: stride %d outside 1..%d", who, s, TRACK_MAX_STRIDE);
  return 0;
}

static int track_batch_check(const char* who, int B) {
  D3F_CHECK(B >= 0 && B <= 65535, "%s: B %d outside 0..65535 frames per call", who, B);
  return 0;
}

static int track_side_check(const char* who, int tw, int th) {
  D3F_CHECK(tw >= TRACK_MIN_SIDE && tw <= TRACK_MAX_SIDE && th >= TRACK_MIN_SIDE && th <= TRACK_MAX_SIDE,
            "%s: template %d x %d outside %d..%d", who, tw, th, TRACK_MIN_SIDE, TRACK_MAX_SIDE);
  return 0;
}

int gray_decimate_check(int B, int h, int w, int s) {
  if (int rc = track_batch_check("gray_decimate", B)) return rc;
  return track_frame_check("gray_decimate", h, w, s);
}

int gray_decimate_u8_launch(const uint8_t* frames, int B, int h, int w, int s, uint8_t* out, hipStream_t stream) {
  if (int rc = gray_decimate_check(B, h, w, s)) return rc;
  const int gh = h / s, gw = w / s;
  if (B == 0 || gh == 0 || gw == 0) return 0;
  const DecimateGeom g = {B, h, w, s, gh, gw};
  hipLaunchKernelGGL(gray_decimate_kernel, dim3((gw + GD_THREADS - 1) / GD_THREADS, gh, B), dim3(GD_THREADS), 0, stream,
                     frames, g, out);
  D3F_HIP(hipGetLastError());
  return 0;
}

int track_seed_u8_launch(const uint8_t* frame, int h, int w, int s, int tx, int ty, int tw, int th, uint8_t* templ, int* pos,
                         bool with_level, hipStream_t stream) {
  if (int rc = track_frame_check("track_seed", h, w, s)) return rc;
  if (int rc = track_side_check("track_seed", tw, th)) return rc;
  D3F_CHECK(tx >= 0 && ty >= 0 && tx + tw <= w / s && ty + th <= h / s,
            "track_seed: box (%d, %d, %d, %d) outside the reduced image %d x %d", tx, ty, tw, th, w / s, h / s);
  D3F_CHECK((reinterpret_cast<uintptr_t>(pos) & 3) == 0, "track_seed: pos must be aligned to 4 bytes");
  hipLaunchKernelGGL(track_seed_kernel, dim3(th), dim3(64), 0, stream, frame, w, s, tx, ty, tw,
                     with_level ? (tw > th ? tw : th) : 0, templ, pos);
  D3F_HIP(hipGetLastError());
  return 0;
}

int track_search_check(int B, int gh, int gw, int tw, int th, int search, int adapt, int lost, const int* pos,
                       const int* out) {
  if (int rc = track_batch_check("track_search", B)) return rc;
  D3F_CHECK(gh > 0 && gw > 0 && gh <= 16384 && gw <= 16384, "track_search: reduced size %d x %d outside 1..16384", gh, gw);
  if (int rc = track_side_check("track_search", tw, th)) return rc;
  D3F_CHECK(gh >= th && gw >= tw, "track_search: template %d x %d larger than the reduced image %d x %d", tw, th, gw, gh);
  D3F_CHECK(search >= 1 && search <= TRACK_MAX_SEARCH, "track_search: search %d outside 1..%d", search, TRACK_MAX_SEARCH);
  D3F_CHECK(adapt >= 0 && adapt <= 8, "track_search: adapt %d outside 0..8", adapt);
  D3F_CHECK(lost >= 0 && lost <= 255, "track_search: lost %d outside 0..255", lost);
  D3F_CHECK(((reinterpret_cast<uintptr_t>(pos) | reinterpret_cast<uintptr_t>(out)) & 3) == 0,
            "track_search: pos and out must be aligned to 4 bytes");
  return 0;
}

int track_search_u8_launch(const uint8_t* gray, int B, int gh, int gw, int tw, int th, int search, int adapt, int lost,
                           uint8_t* templ, int* pos, int* out, hipStream_t stream) {
  if (int rc = track_search_check(B, gh, gw, tw, th, search, adapt, lost, pos, out)) return rc;
  if (B == 0) return 0;
  const SearchGeom g = {B, gh, gw, tw, th, search, adapt, lost};
  hipLaunchKernelGGL(track_search_kernel, dim3(1), dim3(TS_THREADS), 0, stream, gray, g, templ, pos, out);
  D3F_HIP(hipGetLastError());
  return 0;
}

int track_template_u8_launch(const uint8_t* frames, int B, int h, int w, int s, int tw, int th, int search, int adapt,
                             int lost, uint8_t* templ, int* pos, uint8_t* gray_ws, int* out, hipStream_t stream) {
  // both refusals before either launch
  if (int rc = gray_decimate_check(B, h, w, s)) return rc;
  D3F_CHECK(h / s > 0 && w / s > 0, "track_template: stride %d leaves nothing of %d x %d", s, h, w);
  if (int rc = track_search_check(B, h / s, w / s, tw, th, search, adapt, lost, pos, out)) return rc;
  if (int rc = gray_decimate_u8_launch(frames, B, h, w, s, gray_ws, stream)) return rc;
  return track_search_u8_launch(gray_ws, B, h / s, w / s, tw, th, search, adapt, lost, templ, pos, out, stream);
}

int track_global_check(int B, int gh, int gw, int tw, int th, const void* keys) {
  if (int rc = track_batch_check("track_global", B)) return rc;
  D3F_CHECK(gh > 0 && gw > 0 && gh <= 16384 && gw <= 16384, "track_global: reduced size %d x %d outside 1..16384", gh, gw);
  if (int rc = track_side_check("track_global", tw, th)) return rc;
  D3F_CHECK(gh >= th && gw >= tw, "track_global: template %d x %d larger than the reduced image %d x %d", tw, th, gw, gh);
  D3F_CHECK((reinterpret_cast<uintptr_t>(keys) & 7) == 0, "track_global: keys must be aligned to 8 bytes");
  return 0;
}

// two launches: the keys set to all-ones, then the tiles' minima taken into them
int track_global_u8_launch(const uint8_t* gray, int B, int gh, int gw, int tw, int th, const uint8_t* key_templ,
                           unsigned long long* keys, hipStream_t stream) {
  if (int rc = track_global_check(B, gh, gw, tw, th, keys)) return rc;
  if (B == 0) return 0;
  const int ntx = (gw - tw + TG_X) / TG_X, nty = (gh - th + TG_Y) / TG_Y;  // gw - tw + 1 candidates in a row
  const GlobalGeom g = {B, gh, gw, tw, th, ntx};
  hipLaunchKernelGGL(track_keys_fill_kernel, dim3((B + 255) / 256), dim3(256), 0, stream, keys, B);
  D3F_HIP(hipGetLastError());
  hipLaunchKernelGGL(track_global_kernel, dim3(ntx * nty, B), dim3(TG_THREADS), 0, stream, gray, g, key_templ, keys);
  D3F_HIP(hipGetLastError());
  return 0;
}

int track_search_reacq_check(int B, int gh, int gw, int tw, int th, int search, int adapt, int lost, int relost,
                             const uint8_t* templ, const uint8_t* key_templ, const int* pos, const void* keys, const int* out) {
  if (int rc = track_search_check(B, gh, gw, tw, th, search, adapt, lost, pos, out)) return rc;
  D3F_CHECK(relost >= 0 && relost <= 255, "track_search_reacq: relost %d outside 0..255", relost);
  D3F_CHECK((reinterpret_cast<uintptr_t>(keys) & 7) == 0, "track_search_reacq: keys must be aligned to 8 bytes");
  // the tw * th bytes each kernel touches of either template
  D3F_CHECK(key_templ + tw * th <= templ || templ + tw * th <= key_templ,
            "track_search_reacq: key_templ overlaps templ (the key template is never adapted: a buffer of its own)");
  return 0;
}

int track_search_reacq_u8_launch(const uint8_t* gray, int B, int gh, int gw, int tw, int th, int search, int adapt, int lost,
                                 int relost, uint8_t* templ, const uint8_t* key_templ, int* pos,
                                 const unsigned long long* keys, int* out, hipStream_t stream) {
  if (int rc = track_search_reacq_check(B, gh, gw, tw, th, search, adapt, lost, relost, templ, key_templ, pos, keys, out))
    return rc;
  if (B == 0) return 0;
  const SearchGeom g = {B, gh, gw, tw, th, search, adapt, lost};
  hipLaunchKernelGGL(track_search_reacq_kernel, dim3(1), dim3(TS_THREADS), 0, stream, gray, g, templ, pos, out, key_templ, keys,
                     relost);
  D3F_HIP(hipGetLastError());
  return 0;
}

// four launches: the reduced image, the keys' fill, the whole-frame search, the serial search
int track_template_reacq_u8_launch(const uint8_t* frames, int B, int h, int w, int s, int tw, int th, int search, int adapt,
                                   int lost, int relost, uint8_t* templ, const uint8_t* key_templ, int* pos, uint8_t* gray_ws,
                                   unsigned long long* keys_ws, int* out, hipStream_t stream) {
  // every refusal before any launch
  if (int rc = gray_decimate_check(B, h, w, s)) return rc;
  D3F_CHECK(h / s > 0 && w / s > 0, "track_template_reacq: stride %d leaves nothing of %d x %d", s, h, w);
  if (int rc = track_search_reacq_check(B, h / s, w / s, tw, th, search, adapt, lost, relost, templ, key_templ, pos, keys_ws, out))
    return rc;
  if (int rc = gray_decimate_u8_launch(frames, B, h, w, s, gray_ws, stream)) return rc;
  if (int rc = track_global_u8_launch(gray_ws, B, h / s, w / s, tw, th, key_templ, keys_ws, stream)) return rc;
  return track_search_reacq_u8_launch(gray_ws, B, h / s, w / s, tw, th, search, adapt, lost, relost, templ, key_templ, pos,
                                      keys_ws, out, stream);
}

int track_search_scale_check(int B, int gh, int gw, int tw0, int th0, int search, int adapt, int lost, int levels, int penalty,
                             const int* pos, const int* out) {
  if (int rc = track_search_check(B, gh, gw, tw0, th0, search, adapt, lost, pos, out)) return rc;
  D3F_CHECK(levels >= 0 && levels <= 1, "track_search_scale: levels %d outside 0..1", levels);
  D3F_CHECK(penalty >= 0 && penalty <= 65535, "track_search_scale: penalty %d outside 0..65535", penalty);
  return 0;
}

int track_search_scale_u8_launch(const uint8_t* gray, int B, int gh, int gw, int tw0, int th0, int search, int adapt, int lost,
                                 int levels, int penalty, uint8_t* templ, int* pos, int* out, hipStream_t stream) {
  if (int rc = track_search_scale_check(B, gh, gw, tw0, th0, search, adapt, lost, levels, penalty, pos, out)) return rc;
  if (B == 0) return 0;
  // the valid levels around the seed's own, which the check above has found valid: the sizes grow with the level
  const int L0 = tw0 > th0 ? tw0 : th0;
  const auto valid = [&](int L) {
    const int tw = track_level_side(tw0, L, L0), th = track_level_side(th0, L, L0);
    return L >= 1 && tw >= TRACK_MIN_SIDE && th >= TRACK_MIN_SIDE && tw <= TRACK_MAX_SIDE && th <= TRACK_MAX_SIDE && tw <= gw &&
           th <= gh;
  };
  int Lmin = L0, Lmax = L0;
  while (valid(Lmin - 1)) --Lmin;
  while (valid(Lmax + 1)) ++Lmax;
  const ScaleGeom g = {B, gh, gw, tw0, th0, search, adapt, lost, levels, penalty, Lmin, Lmax};
  hipLaunchKernelGGL(track_search_scale_kernel, dim3(1), dim3(TS_THREADS), 0, stream, gray, g, templ, pos, out);
  D3F_HIP(hipGetLastError());
  return 0;
}

int track_template_scale_u8_launch(const uint8_t* frames, int B, int h, int w, int s, int tw0, int th0, int search, int adapt,
                                   int lost, int levels, int penalty, uint8_t* templ, int* pos, uint8_t* gray_ws, int* out,
                                   hipStream_t stream) {
  // both refusals before either launch
  if (int rc = gray_decimate_check(B, h, w, s)) return rc;
  D3F_CHECK(h / s > 0 && w / s > 0, "track_template_scale: stride %d leaves nothing of %d x %d", s, h, w);
  if (int rc = track_search_scale_check(B, h / s, w / s, tw0, th0, search, adapt, lost, levels, penalty, pos, out)) return rc;
  if (int rc = gray_decimate_u8_launch(frames, B, h, w, s, gray_ws, stream)) return rc;
  return track_search_scale_u8_launch(gray_ws, B, h / s, w / s, tw0, th0, search, adapt, lost, levels, penalty, templ, pos, out,
                                      stream);
}

int track_seed_rot_u8_launch(const uint8_t* frame, int h, int w, int s, int tx, int ty, int tw, int th, int a0, int c16, int s16,
                             uint8_t* templ, int* pos, hipStream_t stream) {
  D3F_CHECK(a0 >= -RS_MAX_INDEX && a0 <= RS_MAX_INDEX, "track_seed_rot: angle index %d outside -%d..%d", a0, RS_MAX_INDEX,
            RS_MAX_INDEX);
  D3F_CHECK(abs(c16) <= 65536 && abs(s16) <= 65536, "track_seed_rot: rot (c16 %d, s16 %d) outside -65536..65536", c16, s16);
  // the plain seed's launch (it refuses what it refuses, before anything runs), then the turn and pos[2]
  if (int rc = track_seed_u8_launch(frame, h, w, s, tx, ty, tw, th, templ, pos, false, stream)) return rc;
  hipLaunchKernelGGL(track_seed_rot_kernel, dim3(1), dim3(TS_THREADS), 0, stream, templ, tw, th, a0, c16, s16, pos);
  D3F_HIP(hipGetLastError());
  return 0;
}

int track_search_rot_check(int B, int gh, int gw, int tw0, int th0, int search, int adapt, int lost, int steps, int penalty,
                           int amax, const int* table, const int* pos, const int* out) {
  if (int rc = track_search_check(B, gh, gw, tw0, th0, search, adapt, lost, pos, out)) return rc;
  D3F_CHECK(steps >= 0 && steps <= 1, "track_search_rot: steps %d outside 0..1", steps);
  D3F_CHECK(penalty >= 0 && penalty <= 65535, "track_search_rot: penalty %d outside 0..65535", penalty);
  D3F_CHECK(amax >= 0 && amax <= RS_MAX_INDEX, "track_search_rot: amax %d outside 0..%d", amax, RS_MAX_INDEX);
  D3F_CHECK(table != nullptr, "track_search_rot: null table (host memory [2 amax + 1][2]: c16, s16 per angle index)");
  for (int i = 0; i < 2 * (2 * amax + 1); ++i)
    D3F_CHECK(table[i] >= -65536 && table[i] <= 65536, "track_search_rot: table entry %d (angle index %d) is %d, outside "
              "-65536..65536", i, i / 2 - amax, table[i]);
  return 0;
}

int track_search_rot_u8_launch(const uint8_t* gray, int B, int gh, int gw, int tw0, int th0, int search, int adapt, int lost,
                               int steps, int penalty, int amax, const int* table, uint8_t* templ, int* pos, int* out,
                               hipStream_t stream) {
  if (int rc = track_search_rot_check(B, gh, gw, tw0, th0, search, adapt, lost, steps, penalty, amax, table, pos, out)) return rc;
  if (B == 0) return 0;
  RotGeom g = {B, gh, gw, tw0, th0, search, adapt, lost, steps, penalty, amax, {}};
  for (int i = 0; i < 2 * amax + 1; ++i) g.rot[i] = FrameRot{table[2 * i], table[2 * i + 1]};
  hipLaunchKernelGGL(track_search_rot_kernel, dim3(1), dim3(TS_THREADS), 0, stream, gray, g, templ, pos, out);
  D3F_HIP(hipGetLastError());
  return 0;
}

int track_template_rot_u8_launch(const uint8_t* frames, int B, int h, int w, int s, int tw0, int th0, int search, int adapt,
                                 int lost, int steps, int penalty, int amax, const int* table, uint8_t* templ, int* pos,
                                 uint8_t* gray_ws, int* out, hipStream_t stream) {
  // both refusals before either launch
  if (int rc = gray_decimate_check(B, h, w, s)) return rc;
  D3F_CHECK(h / s > 0 && w / s > 0, "track_template_rot: stride %d leaves nothing of %d x %d", s, h, w);
  if (int rc = track_search_rot_check(B, h / s, w / s, tw0, th0, search, adapt, lost, steps, penalty, amax, table, pos, out))
    return rc;
  if (int rc = gray_decimate_u8_launch(frames, B, h, w, s, gray_ws, stream)) return rc;
  return track_search_rot_u8_launch(gray_ws, B, h / s, w / s, tw0, th0, search, adapt, lost, steps, penalty, amax, table, templ,
                                    pos, out, stream);
}

}  // namespace d3f
