// Counting over a video: how far the scene moved between consecutive frames, and which objects of the next frame continue objects of
// the previous one (include/mgunet.h, "video": THIS BUILD'S DEFINITION, integers only).
//   frame_plane_kernel   uint8 frames (T, H, W, 3 | 1) -> byte planes (T, Hp, pitch): the luma byte (77 R + 150 G + 29 B + 128) >> 8
//                        averaged over f x f blocks with rounding; four pixels per thread, one word store, the pad of a row zeroed
//   frame_sad_kernel     the hot path.  One workgroup = one 48 x 48 tile of the window of one frame pair: the tile of plane t and the
//                        tile plus its search halo of plane t + 1 sit as bytes in LDS (15.3 KB at radius 32).  A lane owns four
//                        consecutive x-shifts of one y-shift and walks the tile four pixels per instruction: the word of plane t is
//                        the same for every lane (an LDS broadcast); the word of plane t + 1 at byte offset j of its aligned word is
//                        formed from two neighbouring words (v_alignbyte_b32), of which one is carried over from the step before; four
//                        v_sad_u8 add into four 32-bit sums (a tile is at most 48 * 48 * 255).  Per word of the tile and lane: 3 align
//                        and 4 SAD instructions for 16 pixel differences; a whole tile is walked a row at a time from registers (3
//                        16-byte reads of A, 13 words of B in flight together), a tile cut by the window's edge word by word with the
//                        last word masked.  A level with more (y-shift, x-group) tasks than lanes is cut along sy into grid.z chunks of
//                        at most 256 tasks; one with fewer (the fine level: radius <= 8) splits the rows of the tile among lanes as
//                        well.  The sums meet in a 32-bit LDS table and go to the 64-bit surface with one integer atomic per shift and
//                        workgroup: exact and order-free.  No masked SAD form: a zero byte counts like any other.
//   frame_pick_kernel    one workgroup per pair: the smallest (cost, sy^2 + sx^2, sy, sx) of the surface
//   track_align_kernel   both label maps of a pair in the next frame's coordinates, cut to the common rectangle, and the visible areas
//   track_ids_kernel     one workgroup walks the frames: an object takes its predecessor's id or the next fresh one (a scan, no atomic)
#include <algorithm>

#include "objects_common.h"

namespace mgu {
namespace {

constexpr int VID_THREADS = 256;
constexpr int VID_TILE = 48;                          // side of a tile of the window, pixels (a multiple of 4)
constexpr int VID_NW = VID_TILE / 4;                  // words per tile row
constexpr int VID_RMAX = 32;                          // largest search radius
constexpr int VID_GMAX = (2 * VID_RMAX + 7) / 4;      // x-shift groups of four: offsets 0 .. 2 r + 3 (the halo starts on a word)
constexpr int VID_PW = VID_GMAX + VID_NW;             // words per halo row in LDS
constexpr int VID_BROWS = VID_TILE + 2 * VID_RMAX;    // halo rows in LDS
constexpr int VID_NSMAX = (2 * VID_RMAX + 1) * (2 * VID_RMAX + 1);

__device__ __forceinline__ unsigned luma_byte(const uint8_t* p, int ch, int bgr) {
  if (ch == 1) return p[0];
  const unsigned r = p[bgr ? 2 : 0], g = p[1], b = p[bgr ? 0 : 2];
  return (77u * r + 150u * g + 29u * b + 128u) >> 8;
}

// thread = four consecutive pixels of one plane row; f = 1 << lf
__global__ __launch_bounds__(VID_THREADS) void frame_plane_kernel(const uint8_t* __restrict__ frames, int T, int H, int W, int ch, int bgr, int lf,
                                                                  int Hp, int Wp, int pitch, uint8_t* __restrict__ out) {
  const int pw = pitch / 4, f = 1 << lf;
  const int64_t n = (int64_t)T * Hp * pw;
  for (int64_t i = (int64_t)blockIdx.x * VID_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * VID_THREADS) {
    const int xw = (int)(i % pw), y = (int)((i / pw) % Hp);
    const int64_t t = i / ((int64_t)pw * Hp);
    const uint8_t* fr = frames + t * (int64_t)H * W * ch;
    unsigned word = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int x = 4 * xw + k;
      if (x >= Wp) break;
      unsigned s = 0;
      for (int dy = 0; dy < f; ++dy)
        for (int dx = 0; dx < f; ++dx) s += luma_byte(fr + ((int64_t)(y * f + dy) * W + (x * f + dx)) * ch, ch, bgr);
      word |= ((s + ((1u << (2 * lf)) >> 1)) >> (2 * lf)) << (8 * k);
    }
    *reinterpret_cast<unsigned*>(out + (t * Hp + y) * (int64_t)pitch + 4 * xw) = word;
  }
}

// One level of the search.  Planes (T, Hp, pitch) bytes, Wp valid bytes a row, every row and plane on a 4-byte boundary.  The window is
// [M, Hp - M) x [M, Wp - M); the shifts are centre + d, d in [-r, r]^2, centre = scale * centre_dev[pair] clamped to [-cmax, cmax]
// (0 without centre_dev).  M >= cmax + r, so no shift reads outside a plane.
struct SadLevel {
  const uint8_t* planes;
  int Hp, Wp, pitch, M, r, scale, cmax;
};

__device__ __forceinline__ int level_centre(const SadLevel& L, const int* __restrict__ centre, int b, int k) {
  if (!centre) return 0;
  const long long v = (long long)centre[2 * b + k] * L.scale;
  return (int)(v < -L.cmax ? -L.cmax : v > L.cmax ? L.cmax : v);
}

__device__ __forceinline__ void sad4(unsigned a, unsigned lo, unsigned hi, unsigned& s0, unsigned& s1, unsigned& s2, unsigned& s3) {
  s0 = __builtin_amdgcn_sad_u8(a, lo, s0);
  s1 = __builtin_amdgcn_sad_u8(a, __builtin_amdgcn_alignbyte(hi, lo, 1), s1);
  s2 = __builtin_amdgcn_sad_u8(a, __builtin_amdgcn_alignbyte(hi, lo, 2), s2);
  s3 = __builtin_amdgcn_sad_u8(a, __builtin_amdgcn_alignbyte(hi, lo, 3), s3);
}

// y-shifts per workgroup: a level with more (y-shift, x-group) tasks than lanes is cut along sy into grid.z chunks of at most
// VID_THREADS tasks, so every lane has one task and the chip has about three times as many workgroups to spread
__host__ __device__ inline int sad_chunk(int r) {
  const int D = 2 * r + 1, G = (2 * r + 7) / 4;
  return D * G <= VID_THREADS ? D : VID_THREADS / G;
}

__global__ __launch_bounds__(VID_THREADS) void frame_sad_kernel(SadLevel L, const int* __restrict__ centre, unsigned long long* __restrict__ surface) {
  __shared__ __attribute__((aligned(16))) unsigned shA[VID_TILE * VID_NW];
  __shared__ unsigned shB[VID_BROWS * VID_PW];
  __shared__ unsigned acc[VID_NSMAX];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int wh = L.Hp - 2 * L.M, ww = L.Wp - 2 * L.M;
  const int tiles_x = (ww + VID_TILE - 1) / VID_TILE;
  const int y0 = L.M + (int)(blockIdx.x / tiles_x) * VID_TILE, x0 = L.M + (int)(blockIdx.x % tiles_x) * VID_TILE;
  const int th = min(VID_TILE, L.M + wh - y0), tw = min(VID_TILE, L.M + ww - x0);
  const int r = L.r, D = 2 * r + 1, NS = D * D, G = (2 * r + 7) / 4, PW = G + VID_NW;
  const int CH = sad_chunk(r), sy_lo = (int)blockIdx.z * CH, nsy = min(CH, D - sy_lo);   // this workgroup's y-shifts: [sy_lo, sy_lo + nsy)
  const int cy = level_centre(L, centre, b, 0), cx = level_centre(L, centre, b, 1);
  const int64_t plane = (int64_t)L.Hp * L.pitch;
  const uint8_t* A = L.planes + b * plane;
  const uint8_t* B = A + plane;
  // the tile of A, bytes past the tile zeroed
  for (int i = tid; i < VID_TILE * VID_NW; i += VID_THREADS) {
    const int y = i / VID_NW, xw = i % VID_NW;
    unsigned word = 0;
    if (y < th)
      for (int k = 0; k < 4; ++k) {
        const int x = 4 * xw + k;
        if (x < tw) word |= (unsigned)A[(int64_t)(y0 + y) * L.pitch + x0 + x] << (8 * k);
      }
    shA[i] = word;
  }
  // the halo of B for this workgroup's y-shifts, from the aligned word at or below its first column: whole words inside the plane's
  // rows, 0 elsewhere.  LDS row y holds plane row by0 + y.
  const int by0 = y0 + cy - r + sy_lo, braw = x0 + cx - r, e = braw & 3, bx0 = braw - e;
  const int brows = th + nsy - 1;
  for (int i = tid; i < brows * PW; i += VID_THREADS) {
    const int y = i / PW, xw = i % PW;
    const int gy = by0 + y, gx = bx0 + 4 * xw;
    unsigned word = 0;
    if (gy >= 0 && gy < L.Hp && gx >= 0 && gx + 4 <= L.pitch) word = *reinterpret_cast<const unsigned*>(B + (int64_t)gy * L.pitch + gx);
    shB[i] = word;
  }
  for (int i = tid; i < nsy * D; i += VID_THREADS) acc[i] = 0;
  __syncthreads();
  // task = (row slice, y-shift, group of four x-offsets); offset o = sx + r + e = 4 g + j
  const int ntask = nsy * G;
  const int S = max(1, min(th, VID_THREADS / ntask));
  const int nfull = tw >> 2, tail = tw & 3;
  const unsigned tmask = tail ? (1u << (8 * tail)) - 1u : 0u;
  for (int task = tid; task < ntask * S; task += VID_THREADS) {
    const int slice = task / ntask, rem = task % ntask, syi = rem / G, g = rem % G;
    const int ya = slice * th / S, yb = (slice + 1) * th / S;
    unsigned s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    if (tw == VID_TILE) {   // a whole row of the tile and of the halo in registers: the loads of a row are in flight together
      for (int y = ya; y < yb; ++y) {
        const uint4* ar = reinterpret_cast<const uint4*>(shA + y * VID_NW);
        const unsigned* br = shB + (y + syi) * PW + g;
        unsigned bw[VID_NW + 1];
#pragma unroll
        for (int x = 0; x <= VID_NW; ++x) bw[x] = br[x];
#pragma unroll
        for (int q = 0; q < VID_NW / 4; ++q) {
          const uint4 a = ar[q];
          sad4(a.x, bw[4 * q], bw[4 * q + 1], s0, s1, s2, s3);
          sad4(a.y, bw[4 * q + 1], bw[4 * q + 2], s0, s1, s2, s3);
          sad4(a.z, bw[4 * q + 2], bw[4 * q + 3], s0, s1, s2, s3);
          sad4(a.w, bw[4 * q + 3], bw[4 * q + 4], s0, s1, s2, s3);
        }
      }
    } else {
      for (int y = ya; y < yb; ++y) {
        const unsigned* ar = shA + y * VID_NW;
        const unsigned* br = shB + (y + syi) * PW + g;
        unsigned lo = br[0];
        for (int x = 0; x < nfull; ++x) {
          const unsigned hi = br[x + 1];
          sad4(ar[x], lo, hi, s0, s1, s2, s3);
          lo = hi;
        }
        if (tail) {   // the last 1..3 columns: the bytes past the tile are 0 on both sides
          const unsigned a = ar[nfull], hi = br[nfull + 1];
          s0 = __builtin_amdgcn_sad_u8(a, lo & tmask, s0);
          s1 = __builtin_amdgcn_sad_u8(a, __builtin_amdgcn_alignbyte(hi, lo, 1) & tmask, s1);
          s2 = __builtin_amdgcn_sad_u8(a, __builtin_amdgcn_alignbyte(hi, lo, 2) & tmask, s2);
          s3 = __builtin_amdgcn_sad_u8(a, __builtin_amdgcn_alignbyte(hi, lo, 3) & tmask, s3);
        }
      }
    }
    const unsigned sums[4] = {s0, s1, s2, s3};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int sxi = 4 * g + j - e;
      if (sxi >= 0 && sxi < D && sums[j]) atomicAdd(&acc[syi * D + sxi], sums[j]);
    }
  }
  __syncthreads();
  for (int i = tid; i < nsy * D; i += VID_THREADS)
    if (acc[i]) atomicAdd(&surface[(int64_t)b * NS + sy_lo * D + i], (unsigned long long)acc[i]);
}

// The smallest cost; ties: the smallest sy^2 + sx^2, then the smaller sy, then the smaller sx -- entry i = (sy + r) * D + (sx + r) ascends
// in (sy, sx), so the key is (cost, sy^2 + sx^2, i).  shift_out[pair] = centre + d; cost_out[pair] = [cost there, cost at d = 0].
__global__ __launch_bounds__(VID_THREADS) void frame_pick_kernel(SadLevel L, const int* __restrict__ centre,
                                                                 const unsigned long long* __restrict__ surface, int* __restrict__ shift_out,
                                                                 long long* __restrict__ cost_out) {
  __shared__ unsigned long long shc[VID_THREADS];
  __shared__ int shd[VID_THREADS], shi[VID_THREADS];
  const int tid = threadIdx.x, b = blockIdx.x, r = L.r, D = 2 * r + 1, NS = D * D;
  const unsigned long long* sf = surface + (int64_t)b * NS;
  unsigned long long bc = ~0ull;
  int bd = INT_MAX, bi = INT_MAX;
  for (int i = tid; i < NS; i += VID_THREADS) {
    const int sy = i / D - r, sx = i % D - r, d2 = sy * sy + sx * sx;
    const unsigned long long c = sf[i];
    if (c < bc || (c == bc && (d2 < bd || (d2 == bd && i < bi)))) bc = c, bd = d2, bi = i;
  }
  shc[tid] = bc, shd[tid] = bd, shi[tid] = bi;
  __syncthreads();
  for (int off = VID_THREADS / 2; off > 0; off >>= 1) {
    if (tid < off) {
      const unsigned long long c = shc[tid + off];
      const int d2 = shd[tid + off], i = shi[tid + off];
      if (c < shc[tid] || (c == shc[tid] && (d2 < shd[tid] || (d2 == shd[tid] && i < shi[tid])))) shc[tid] = c, shd[tid] = d2, shi[tid] = i;
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int i = shi[0];
    shift_out[2 * b] = level_centre(L, centre, b, 0) + i / D - r;
    shift_out[2 * b + 1] = level_centre(L, centre, b, 1) + i % D - r;
    if (cost_out) cost_out[2 * b] = (long long)shc[0], cost_out[2 * b + 1] = (long long)sf[r * D + r];
  }
}

// pair b = frames (b, b + 1), s = shifts[b]: prev[q] = labels_b[q - s] inside the frame, else 0; next[q] = labels_{b+1}[q] where q - s lies
// inside the frame (the common rectangle), else 0.  Visible areas: one integer add per wave and object.
__global__ __launch_bounds__(VID_THREADS) void track_align_kernel(const int* __restrict__ labels, const long long* __restrict__ off, int64_t cap,
                                                                  const int* __restrict__ shifts, int64_t n, int H, int W, int* __restrict__ prev,
                                                                  int* __restrict__ next, unsigned long long* __restrict__ vis_prev,
                                                                  unsigned long long* __restrict__ vis_next) {
  const int64_t HW = (int64_t)H * W;
  auto add = [](unsigned long long* vis, long long key) {
    wave_by_key(
        key,
        [=](long long k, bool mine, bool lead) {
          const unsigned long long cnt = (unsigned long long)__popcll(__ballot(mine));
          if (lead) atomicAdd(&vis[k], cnt);
        },
        [=] { atomicAdd(&vis[key], 1ull); });
  };
  for (int64_t base = (int64_t)blockIdx.x * VID_THREADS; base < n; base += (int64_t)gridDim.x * VID_THREADS) {
    const int64_t i = base + threadIdx.x;
    long long kp = -1, kn = -1;
    if (i < n) {
      const int64_t b = i / HW, q = i % HW;
      const long long y = q / W, x = q % W, py = y - shifts[2 * b], px = x - shifts[2 * b + 1];
      int pa = 0, nc = 0;
      if (py >= 0 && py < H && px >= 0 && px < W) pa = labels[b * HW + py * W + px], nc = labels[(b + 1) * HW + q];
      prev[i] = pa, next[i] = nc;
      if (pa > 0 && pa <= off[b + 1] - off[b]) kp = object_index(pa, off, b, cap);
      if (nc > 0 && nc <= off[b + 2] - off[b + 1]) kn = object_index(nc, off, b + 1, cap);
    }
    add(vis_prev, kp);
    add(vis_next, kn);
  }
}

// One workgroup, frame after frame.  Frame 0 takes first_ids (and is then not counted: the chunk before counted it) or fresh ids; a later
// object takes the id of link[i] (an object of an earlier frame) or a fresh one: next + its rank among the frame's unlinked objects.
__global__ __launch_bounds__(VID_THREADS) void track_ids_kernel(const long long* __restrict__ off, int T, int64_t cap, const long long* __restrict__ link,
                                                                const long long* __restrict__ cls, const long long* __restrict__ first_ids,
                                                                long long* next_id, long long* track_id, int* __restrict__ track_len,
                                                                long long* __restrict__ track_cls, int64_t tcap, int* __restrict__ status) {
  __shared__ int sh[4];
  const int tid = threadIdx.x;
  long long next = *next_id;
  int bits = 0;
  for (int t = 0; t < T; ++t) {
    const long long o0 = off[t];
    long long n = off[t + 1] - o0;
    if (o0 + n > cap) n = cap > o0 ? cap - o0 : 0, bits |= 2;
    const bool carried = t == 0 && first_ids;
    for (long long base = 0; base < n; base += VID_THREADS) {
      const long long i = base + tid;
      const bool active = i < n;
      long long id = -1;
      int fresh = 0;
      if (active) {
        if (carried) {
          id = first_ids[i];
        } else {
          const long long l = t == 0 ? -1 : link[o0 + i];
          if (l >= 0 && l < o0) id = track_id[l];
          else fresh = 1;
        }
      }
      int total;
      const int rank = block_exclusive_scan(fresh, sh, &total);
      if (fresh) id = next + rank;
      if (active) {
        track_id[o0 + i] = id;
        if (!carried) {
          if (id >= 0 && id < tcap) {
            atomicAdd(&track_len[id], 1);
            if (fresh) track_cls[id] = cls[o0 + i];
          } else {
            bits |= 1;
          }
        }
      }
      next += total;
    }
    __syncthreads();   // the ids of this frame are read by the next one
  }
  if (tid == 0) *next_id = next;
  if (bits) atomicOr(status, bits);
}

}  // namespace
}  // namespace mgu

using namespace mgu;
using namespace mgud;

namespace {

// the fill of a level's surface, its SAD launch and its pick launch
int run_level(mgu_ctx* c, const SadLevel& L, int P, const int* centre, unsigned long long* surface, int* shift_out, long long* cost_out, hipStream_t s) {
  const int D = 2 * L.r + 1;
  HIPCHK(c, hipMemsetAsync(surface, 0, (size_t)P * D * D * sizeof(unsigned long long), s));
  const int wh = L.Hp - 2 * L.M, ww = L.Wp - 2 * L.M;
  const unsigned tiles = (unsigned)(((wh + VID_TILE - 1) / VID_TILE) * ((ww + VID_TILE - 1) / VID_TILE));
  {
    ProfScope ps(c, s, "video sad");
    hipLaunchKernelGGL(frame_sad_kernel, dim3(tiles, (unsigned)P, (unsigned)((D + sad_chunk(L.r) - 1) / sad_chunk(L.r))), dim3(VID_THREADS), 0, s, L, centre,
                       surface);
  }
  {
    ProfScope ps(c, s, "video pick");
    hipLaunchKernelGGL(frame_pick_kernel, dim3((unsigned)P), dim3(VID_THREADS), 0, s, L, centre, (const unsigned long long*)surface, shift_out, cost_out);
  }
  return MGU_OK;
}

int plane_launch(mgu_ctx* c, const uint8_t* frames, int T, int H, int W, int ch, int bgr, int lf, int Hp, int Wp, int pitch, uint8_t* out, hipStream_t s) {
  ProfScope ps(c, s, "video planes");
  hipLaunchKernelGGL(frame_plane_kernel, dim3((unsigned)grid_for((int64_t)T * Hp * (pitch / 4), VID_THREADS, 256 * 32)), dim3(VID_THREADS), 0, s, frames, T,
                     H, W, ch, bgr ? 1 : 0, lf, Hp, Wp, pitch, out);
  return MGU_OK;
}

}  // namespace

extern "C" {

int mgu_frame_sad_tile(void) { return VID_TILE; }

int mgu_frame_shifts(mgu_ctx* c, const uint8_t* frames_u8, int T, int H, int W, int channels, int bgr, int radius, int factor, int32_t* shifts_dev,
                     int64_t* cost_dev, int64_t* surface_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!frames_u8 || !shifts_dev || !cost_dev) return fail(c, MGU_ERR_INVALID, "frame_shifts: null pointer (frames, shifts_dev or cost_dev)");
  if (T < 2 || T > 65536) return fail(c, MGU_ERR_INVALID, "frame_shifts: 2 <= T <= 65536 frames, got %d", T);
  if (channels != 1 && channels != 3) return fail(c, MGU_ERR_INVALID, "frame_shifts: 1 or 3 channels, got %d", channels);
  if (radius < 1 || radius > VID_RMAX) return fail(c, MGU_ERR_INVALID, "frame_shifts: 1 <= radius <= %d, got %d", VID_RMAX, radius);
  if (factor != 1 && factor != 2 && factor != 4 && factor != 8) return fail(c, MGU_ERR_INVALID, "frame_shifts: factor must be 1, 2, 4 or 8, got %d", factor);
  if (H < 1 || W < 1 || H > 16384 || W > 16384) return fail(c, MGU_ERR_INVALID, "frame_shifts: 1 <= H, W <= 16384, got %d x %d", H, W);
  const int Hc = H / factor, Wc = W / factor;
  if (Hc - 2 * radius < 8 || Wc - 2 * radius < 8)
    return fail(c, MGU_ERR_INVALID, "frame_shifts: the coarse plane %d x %d leaves a window under 8 x 8 at radius %d (need H, W >= %d)", Hc, Wc, radius,
                factor * (2 * radius + 8));
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  const int P = T - 1, lf = factor == 1 ? 0 : factor == 2 ? 1 : factor == 4 ? 2 : 3;
  const int pitch_c = rup(Wc, 4), pitch_f = rup(W, 4), Dc = 2 * radius + 1, Df = 2 * factor + 1;
  Carve cv;
  const size_t oC = cv.take((size_t)T * Hc * pitch_c), oF = cv.take(factor > 1 ? (size_t)T * H * pitch_f : 0);
  const size_t oSc = cv.take(surface_dev ? 0 : (size_t)P * Dc * Dc * 8), oSf = cv.take(factor > 1 ? (size_t)P * Df * Df * 8 : 0), oCe = cv.take((size_t)P * 8);
  int rc = ensure(c, &c->imgws, &c->imgws_bytes, cv.off);
  if (rc) return rc;
  char* ws = (char*)c->imgws;
  unsigned long long* surf_c = surface_dev ? (unsigned long long*)surface_dev : (unsigned long long*)(ws + oSc);
  int* centre = (int*)(ws + oCe);
  if ((rc = plane_launch(c, frames_u8, T, H, W, channels, bgr, lf, Hc, Wc, pitch_c, (uint8_t*)(ws + oC), s))) return rc;
  const SadLevel coarse{(const uint8_t*)(ws + oC), Hc, Wc, pitch_c, radius, radius, 0, 0};
  if (factor == 1) {
    if ((rc = run_level(c, coarse, P, nullptr, surf_c, shifts_dev, (long long*)cost_dev, s))) return rc;
  } else {
    if ((rc = run_level(c, coarse, P, nullptr, surf_c, centre, nullptr, s))) return rc;
    if ((rc = plane_launch(c, frames_u8, T, H, W, channels, bgr, 0, H, W, pitch_f, (uint8_t*)(ws + oF), s))) return rc;
    const SadLevel fine{(const uint8_t*)(ws + oF), H, W, pitch_f, factor * radius + factor, factor, factor, factor * radius};
    if ((rc = run_level(c, fine, P, centre, (unsigned long long*)(ws + oSf), shifts_dev, (long long*)cost_dev, s))) return rc;
  }
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_track_align(mgu_ctx* c, const int32_t* labels_dev, const int64_t* offsets_dev, int64_t capacity, const int32_t* shifts_dev, int T, int H, int W,
                    int32_t* prev_aligned_dev, int32_t* next_cropped_dev, int64_t* vis_prev_dev, int64_t* vis_next_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!labels_dev || !offsets_dev || !shifts_dev || !prev_aligned_dev || !next_cropped_dev || T < 2 || H < 1 || W < 1 || capacity < 0)
    return fail(c, MGU_ERR_INVALID, "bad track_align args (null pointer, T < 2, an empty frame or a negative capacity)");
  if (capacity > 0 && (!vis_prev_dev || !vis_next_dev)) return fail(c, MGU_ERR_INVALID, "track_align: the area arrays are needed for a nonzero capacity");
  if (int rc = check_pixel_count(c, "track_align", T, H, W)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  if (capacity > 0) {
    HIPCHK(c, hipMemsetAsync(vis_prev_dev, 0, (size_t)capacity * 8, s));
    HIPCHK(c, hipMemsetAsync(vis_next_dev, 0, (size_t)capacity * 8, s));
  }
  const int64_t n = (int64_t)(T - 1) * H * W;
  {
    ProfScope ps(c, s, "track align");
    hipLaunchKernelGGL(track_align_kernel, dim3((unsigned)grid_for(n, VID_THREADS, 256 * 32)), dim3(VID_THREADS), 0, s, labels_dev,
                       (const long long*)offsets_dev, capacity, shifts_dev, n, H, W, prev_aligned_dev, next_cropped_dev,
                       (unsigned long long*)vis_prev_dev, (unsigned long long*)vis_next_dev);
  }
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_track_ids(mgu_ctx* c, const int64_t* offsets_dev, int T, int64_t capacity, const int64_t* link_dev, const int64_t* class_dev,
                  const int64_t* first_ids_dev, int64_t* next_id_dev, int64_t* track_id_dev, int32_t* track_len_dev, int64_t* track_class_dev,
                  int64_t track_capacity, int32_t* status_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!offsets_dev || !next_id_dev || !status_dev || T < 1 || capacity < 0 || track_capacity < 0)
    return fail(c, MGU_ERR_INVALID, "bad track_ids args (null pointer, T < 1 or a negative capacity)");
  if (capacity > 0 && (!link_dev || !class_dev || !track_id_dev)) return fail(c, MGU_ERR_INVALID, "track_ids: the per-object arrays are needed for a nonzero capacity");
  if (track_capacity > 0 && (!track_len_dev || !track_class_dev)) return fail(c, MGU_ERR_INVALID, "track_ids: the per-track arrays are needed for a nonzero track_capacity");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  {
    ProfScope ps(c, s, "track ids");
    hipLaunchKernelGGL(track_ids_kernel, dim3(1), dim3(VID_THREADS), 0, s, (const long long*)offsets_dev, T, capacity, (const long long*)link_dev,
                       (const long long*)class_dev, (const long long*)first_ids_dev, (long long*)next_id_dev, (long long*)track_id_dev,
                       (int*)track_len_dev, (long long*)track_class_dev, track_capacity, (int*)status_dev);
  }
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
