// Weight-form packers: every form a convolution kernel reads its weights in is written here, from the reference's parameter
// layouts (Conv2d OIHW, ConvTranspose2d (Cin, Cout, 2, 2)).  One element loop ("body") per form, callable with a VIRTUAL
// (block, grid); a form to pack is a PackItem (common.h), built by the form's constructor below; pack_item dispatches an item to
// its body.  Two kernels run items: pack_batch_kernel runs a whole table of them in one launch (a train step repacks every form
// after each optimizer step: the small launches of the U-Net cost more in launch gaps than in work), pack_one_kernel a single item
// passed by value.  Every element of a form is written by exactly one thread, so the bytes do not depend on the grid.
#include "common.h"

#include <algorithm>

namespace mgu {

enum { PACK_WINO, PACK_FIRST_W, PACK_CONVT_X3, PACK_BIAS_TILE, PACK_DGRAD_PANEL, PACK_FIRST_MFMA, PACK_CONV_PANEL, PACK_CONVT_PANEL,
       PACK_CONVT_BF16F, PACK_CONVT_DGRAD_PANEL };

// ---- bodies ---------------------------------------------------------------------------------------------------------------

// Winograd U = G g G^T of wino3x3_f32_kernel / wino3x3_cp_kernel (wino_f32.hip) and the assembly kernels (wino_asm.hip):
// U[ntile][cin/8][i*4+j][lane (h = lane>>5, r = lane&31)][t]  =  (G g G^T)[i][j]  of  cout = 32*ntile + r,
// cin = 8*(cin/8) + 4*h + t.   dgrad = 1: the data-gradient conv, g'[u][v] = w[c][n][2-u][2-v] (roles swapped).
//
// prec = 1 (three bf16 pieces):  Ux[ntile][cin/16][i*4+j][piece][lane (h = lane>>5, r = lane&31)][e]  (uint16),
// cout = 32*ntile + r, cin = 16*(cin/16) + 8*h + e: the B fragment of v_mfma_f32_32x32x16_bf16, one 16-byte lane load.
__device__ __forceinline__ void pack_wino_w_body(const float* __restrict__ w, float* __restrict__ U, int Cout, int Cin, int Cp, int Np,
                                                 int dgrad, int prec, unsigned vblock, unsigned vgrid) {
  if (prec == 1) {
    // Three-piece layout, store-coalesced: a thread owns output channel n and EIGHT consecutive input channels, i.e. one whole
    // 16-byte lane entry of every (component, piece) fragment; lane & 31 = n & 31 and lane >> 5 = the 8-channel half, so a wave's
    // store instruction writes one contiguous 1-KB fragment (a thread per (n, c) wrote 2-byte pieces 1 KB apart: 1.1 TB/s on the
    // 164 MB a train step re-packs).
    const int nC = Cp >> 4;
    const int64_t total8 = (int64_t)Np * (Cp >> 3);
    for (int64_t idx = vblock * (int64_t)blockDim.x + threadIdx.x; idx < total8; idx += (int64_t)vgrid * blockDim.x) {
      const int lane = (int)(idx & 63);
      const int64_t grp = idx >> 6;
      const int c16 = (int)(grp % nC), ntile = (int)(grp / nC);
      const int n = ntile * 32 + (lane & 31), c0 = c16 * 16 + (lane >> 5) * 8;
      float g[8][3][3];
#pragma unroll
      for (int e = 0; e < 8; ++e)
#pragma unroll
        for (int u = 0; u < 3; ++u)
#pragma unroll
          for (int v = 0; v < 3; ++v) {
            const int c = c0 + e;
            float x = 0.f;
            if (n < Cout && c < Cin)
              x = dgrad ? w[(((int64_t)c * Cout + n) * 3 + (2 - u)) * 3 + (2 - v)] : w[(((int64_t)n * Cin + c) * 3 + u) * 3 + v];
            g[e][u][v] = x;
          }
      u32x4* dst = reinterpret_cast<u32x4*>(U) + ((int64_t)ntile * nC + c16) * 16 * 192 + lane;   // [comp][piece][64 lanes] x 16 B
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          unsigned short p0[8], p1[8], p2[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            float t3[3];   // row i of G g: t[i][v]
#pragma unroll
            for (int v = 0; v < 3; ++v)
              t3[v] = i == 0 ? g[e][0][v] : i == 3 ? g[e][2][v] : 0.5f * (g[e][0][v] + (i == 1 ? g[e][1][v] : -g[e][1][v]) + g[e][2][v]);
            const float uv = j == 0 ? t3[0] : j == 3 ? t3[2] : 0.5f * (t3[0] + (j == 1 ? t3[1] : -t3[1]) + t3[2]);
            const unsigned b0 = __float_as_uint(uv) & 0xffff0000u;
            const float r1 = uv - __uint_as_float(b0);               // exact
            const unsigned b1 = __float_as_uint(r1) & 0xffff0000u;
            const float r2 = r1 - __uint_as_float(b1);               // exact; 8 significant bits are left
            p0[e] = (unsigned short)(b0 >> 16), p1[e] = (unsigned short)(b1 >> 16), p2[e] = (unsigned short)(__float_as_uint(r2) >> 16);
          }
          u32x4 q0, q1, q2;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            q0[e] = (unsigned)p0[2 * e] | ((unsigned)p0[2 * e + 1] << 16);
            q1[e] = (unsigned)p1[2 * e] | ((unsigned)p1[2 * e + 1] << 16);
            q2[e] = (unsigned)p2[2 * e] | ((unsigned)p2[2 * e + 1] << 16);
          }
          u32x4* q = dst + (i * 4 + j) * 192;
          q[0] = q0, q[64] = q1, q[128] = q2;
        }
    }
    return;
  }
  const int64_t total = (int64_t)Np * Cp;
  for (int64_t idx = vblock * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)vgrid * blockDim.x) {
    const int c = (int)(idx % Cp), n = (int)(idx / Cp);
    float g[3][3];
#pragma unroll
    for (int u = 0; u < 3; ++u)
#pragma unroll
      for (int v = 0; v < 3; ++v) {
        float x = 0.f;
        if (n < Cout && c < Cin) {
          // forward: w is (Cout, Cin, 3, 3) and n = cout, c = cin.  dgrad: the layer's weight is (C_layer_out = Cin here,
          // C_layer_in = Cout here, 3, 3): output channel n of the dgrad conv is the layer's input channel.
          x = dgrad ? w[(((int64_t)c * Cout + n) * 3 + (2 - u)) * 3 + (2 - v)] : w[(((int64_t)n * Cin + c) * 3 + u) * 3 + v];
        }
        g[u][v] = x;
      }
    float t[4][3];
#pragma unroll
    for (int v = 0; v < 3; ++v) {
      t[0][v] = g[0][v];
      t[1][v] = 0.5f * (g[0][v] + g[1][v] + g[2][v]);
      t[2][v] = 0.5f * (g[0][v] - g[1][v] + g[2][v]);
      t[3][v] = g[2][v];
    }
    float u[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      u[i][0] = t[i][0];
      u[i][1] = 0.5f * (t[i][0] + t[i][1] + t[i][2]);
      u[i][2] = 0.5f * (t[i][0] - t[i][1] + t[i][2]);
      u[i][3] = t[i][2];
    }
    float* dst = U + (((int64_t)(n >> 5) * (Cp >> 3) + (c >> 3)) * 16) * 256 + ((((c >> 2) & 1) * 32 + (n & 31)) * 4 + (c & 3));
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) dst[(i * 4 + j) * 256] = u[i][j];
  }
}

// wf[tap][c][co] = w[co][c][tap] (OIHW), zero for c >= Cin  (conv3x3_first_kernel, elementwise.hip)
__device__ __forceinline__ void pack_first_w_body(const float* __restrict__ w, float* __restrict__ wf, int Cout, int Cin, unsigned vblock,
                                                  unsigned vgrid) {
  const int total = 9 * 4 * Cout;
  for (int i = (int)(vblock * blockDim.x + threadIdx.x); i < total; i += (int)(vgrid * blockDim.x)) {
    const int co = i % Cout, c = (i / Cout) % 4, tap = i / (4 * Cout);
    wf[i] = c < Cin ? w[((int64_t)co * Cin + c) * 9 + tap] : 0.f;
  }
}

// shift[rep * C + c] = bias[c]: the bias as the epilogue shift of a layer without BatchNorm, once per 2x2 tap of a ConvTranspose
// (every kernel that takes IgemmDesc::shift, igemm.hip)
__device__ __forceinline__ void pack_bias_tile_body(const float* __restrict__ bias, float* __restrict__ shift, int C, int reps, unsigned vblock,
                                                    unsigned vgrid) {
  for (int i = (int)(vblock * blockDim.x + threadIdx.x); i < C * reps; i += (int)(vgrid * blockDim.x)) shift[i] = bias[i % C];
}

// Three-piece fragment weights of the fp32 ConvTranspose (convt2x2_x3_kernel, convt_x3.hip):
//   Wx[n / 128][k / 16][(n / 32) & 3][piece][lane = 32 * ((k / 8) & 1) + (n & 31)][k & 7]   (uint16 bf16 bit patterns)
// forward (dgrad = 0): n = (dy * 2 + dx) * Cout + co (the column order of the pixel-shuffle store), k = ci;
// data gradient (dgrad = 1): k = q * Cout + co (q = qy * 2 + qx), n = ci; columns past Cin inside the last 128-column block are never
// read (a 64-column workgroup tile reads its own half).  w is nn.ConvTranspose2d's (Cin, Cout, 2, 2).
__device__ __forceinline__ void pack_convt_x3_body(const float* __restrict__ w, uint16_t* __restrict__ Wx, int Cin, int Cout, int dgrad,
                                                   unsigned vblock, unsigned vgrid) {
  const int K = dgrad ? 4 * Cout : Cin;
  const int64_t total = (int64_t)Cin * Cout * 4;
  const int ksteps = K >> 4;
  for (int64_t idx = vblock * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)vgrid * blockDim.x) {
    const int k = (int)(idx % K), n = (int)(idx / K);
    const int q = dgrad ? k / Cout : n / Cout;
    const int co = dgrad ? k - q * Cout : n - q * Cout;
    const int ci = dgrad ? n : k;
    const float x = w[(((int64_t)ci * Cout + co) * 2 + (q >> 1)) * 2 + (q & 1)];
    const unsigned b0 = __float_as_uint(x) & 0xffff0000u;
    const float r1 = x - __uint_as_float(b0);            // exact
    const unsigned b1 = __float_as_uint(r1) & 0xffff0000u;
    const float r2 = r1 - __uint_as_float(b1);           // exact; 8 significant bits are left
    const int lane = ((k >> 3) & 1) * 32 + (n & 31);
    uint16_t* dst = Wx + (((((int64_t)(n >> 7) * ksteps + (k >> 4)) * 4 + ((n >> 5) & 3)) * 3) * 64 + lane) * 8 + (k & 7);
    dst[0] = (uint16_t)(b0 >> 16);
    dst[512] = (uint16_t)(b1 >> 16);
    dst[1024] = (uint16_t)(__float_as_uint(r2) >> 16);
  }
}

// Three-piece weights of conv3x3_first_mfma_kernel (first_mfma.hip) in fragment order: [k step s][piece][lane][8] bf16 bit patterns;
// lane = 32 h + cout, element e of k step s = slot j = 8 s + e of half h = (tap 5 h + j / 3, channel j % 3); slots without a value
// (j = 15, taps > 8, channels >= Cin) are zero.  w is OIHW (32, Cin, 3, 3).
__device__ __forceinline__ void pack_first_mfma_body(const float* __restrict__ w, uint16_t* __restrict__ wfm, int Cout, int Cin, unsigned vblock,
                                                     unsigned vgrid) {
  for (int i = (int)(vblock * blockDim.x + threadIdx.x); i < 2 * 64 * 8; i += (int)(vgrid * blockDim.x)) {
    const int e = i & 7, lane = (i >> 3) & 63, s = i >> 9;
    const int co = lane & 31, h = lane >> 5, j = 8 * s + e;
    const int tap = 5 * h + j / 3, ch = j % 3;
    float x = 0.f;
    if (j < 15 && tap < 9 && ch < Cin && co < Cout) x = w[((int64_t)co * Cin + ch) * 9 + tap];
    const unsigned b0 = __float_as_uint(x) & 0xffff0000u;
    const float r1 = x - __uint_as_float(b0);            // exact
    const unsigned b1 = __float_as_uint(r1) & 0xffff0000u;
    const float r2 = r1 - __uint_as_float(b1);           // exact; 8 significant bits are left
    uint16_t* dst = wfm + ((size_t)(s * 3) * 64 + lane) * 8 + e;
    dst[0] = (uint16_t)(b0 >> 16);
    dst[512] = (uint16_t)(b1 >> 16);
    dst[1024] = (uint16_t)(__float_as_uint(r2) >> 16);
  }
}

// data-gradient panel of a conv3x3 / 1x1 (the direct kernels of igemm.hip on dgrad_desc's descriptor): din = conv(dz, W') with
// W'[ci][(2-r,2-s), co] = W[co][ci][r][s]: panel [Cin][Kp], k = tap' * Cop + co  (Cop = Cout rounded up to 4, zero padded)
__device__ __forceinline__ void pack_dgrad_w_body(const float* __restrict__ w, float* __restrict__ wp, int Cout, int Cin, int Cop, int KS, int Kp,
                                                  unsigned vblock, unsigned vgrid) {
  const int64_t total = (int64_t)Cin * Kp;
  for (int64_t i = vblock * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)vgrid * blockDim.x) {
    const int ci = (int)(i / Kp), k = (int)(i - (int64_t)ci * Kp);
    const int tap = k / Cop, co = k - tap * Cop;
    float v = 0.f;
    if (tap < KS * KS && co < Cout) v = w[((int64_t)co * Cin + ci) * KS * KS + (KS * KS - 1 - tap)];
    wp[i] = v;
  }
}

// direct panel of a Conv2d (the implicit-GEMM kernels of igemm.hip, IgemmDesc::w; the GAT projection's GEMM reads the same form):
// OIHW (Cout,Cin,KS,KS) -> panel [Cout][Kp], k = (r*KS+s)*Cp + c (zero padded), stored as T
template <typename T>
__device__ __forceinline__ void pack_conv_w_body(const float* __restrict__ w, T* __restrict__ wp, int Cout, int Cin, int Cp, int KS, int Kp,
                                                 unsigned vblock, unsigned vgrid) {
  const int64_t total = (int64_t)Cout * Kp;
  for (int64_t i = vblock * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)vgrid * blockDim.x) {
    const int n = (int)(i / Kp), k = (int)(i - (int64_t)n * Kp);
    const int tap = k / Cp, c = k - tap * Cp;
    float v = 0.f;
    if (tap < KS * KS && c < Cin) v = w[((int64_t)n * Cin + c) * KS * KS + tap];
    wp[i] = (T)v;
  }
}

// direct panel of a ConvTranspose2d (the tile kernels of igemm.hip, out_mode 1): (Cin,Cout,2,2) -> panel [(dy*2+dx)*Cout + co][Kp],
// k = ci, stored as T
template <typename T>
__device__ __forceinline__ void pack_convt_w_body(const float* __restrict__ w, T* __restrict__ wp, int Cin, int Cout, int Kp, unsigned vblock,
                                                  unsigned vgrid) {
  const int64_t total = (int64_t)4 * Cout * Kp;
  for (int64_t i = vblock * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)vgrid * blockDim.x) {
    const int n = (int)(i / Kp), k = (int)(i - (int64_t)n * Kp);
    const int q = n / Cout, co = n - q * Cout;
    wp[i] = (T)((k < Cin) ? w[((int64_t)k * Cout + co) * 4 + q] : 0.f);
  }
}

// bf16 fragments of the bf16-storage ConvTranspose (convt2x2_bf16_kernel, convt_bf16.hip):
// Wf[n / 128][k / 16][(n / 32) & 3][lane = 32 * ((k / 8) & 1) + (n & 31)][k & 7] = bf16(w[ci = k][co][dy][dx]),  n = (dy*2+dx)*Cout + co:
// the B fragment of v_mfma_f32_32x32x16_bf16, one 16-byte lane load
__device__ __forceinline__ void pack_convt_bf16f_body(const float* __restrict__ w, __bf16* __restrict__ Wf, int Cin, int Cout, unsigned vblock,
                                                      unsigned vgrid) {
  const int64_t total = (int64_t)Cin * Cout * 4;
  const int ksteps = Cin >> 4;
  for (int64_t idx = vblock * (int64_t)blockDim.x + threadIdx.x; idx < total; idx += (int64_t)vgrid * blockDim.x) {
    const int k = (int)(idx % Cin), n = (int)(idx / Cin);
    const int q = n / Cout, co = n - q * Cout;
    const float x = w[(((int64_t)k * Cout + co) * 2 + (q >> 1)) * 2 + (q & 1)];
    const int lane = ((k >> 3) & 1) * 32 + (n & 31);
    Wf[(((((int64_t)(n >> 7) * ksteps + (k >> 4)) * 4 + ((n >> 5) & 3))) * 64 + lane) * 8 + (k & 7)] = (__bf16)x;
  }
}

// data-gradient panel of a ConvTranspose2d (the tile kernels of igemm.hip on the KS = 2 gather descriptor):
// dprev[m][ci] = sum_{q,co} dup[pix(m,q)][co] * W[ci][co][q]: panel [Cin][Kp], k = q*Cout + co
__device__ __forceinline__ void pack_convt_dgrad_w_body(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cout, int Kp,
                                                        unsigned vblock, unsigned vgrid) {
  const int64_t total = (int64_t)Cin * Kp;
  for (int64_t i = vblock * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)vgrid * blockDim.x) {
    const int ci = (int)(i / Kp), k = (int)(i - (int64_t)ci * Kp);
    const int q = k / Cout, co = k - q * Cout;
    wp[i] = (q < 4) ? w[((int64_t)ci * Cout + co) * 4 + q] : 0.f;
  }
}

// ---- sizes of the forms, in floats ------------------------------------------------------------------------------------------
// n tiles padded to pairs; 6 bytes per value in the three-piece layout (sized for either)
size_t wino_u_floats(int Cout, int Cp) { return (size_t)((Cout + 63) / 64 * 64) * Cp * 24; }
size_t convt_x3_floats(int Cin, int Cout) { return (size_t)Cin * Cout * 6; }   // 4 Cout columns x Cin x 3 pieces x 2 bytes
size_t convt_x3_dgrad_floats(int Cin, int Cout) { return (size_t)((Cin + 127) / 128 * 128) * Cout * 6; }   // x 4 taps x 3 pieces x 2 B / 4
size_t convt_bf16f_floats(int Cin, int Cout) { return (size_t)Cin * Cout * 2; }   // 4 Cout columns x Cin x 2 bytes
size_t first_mfma_floats() { return 2 * 3 * 64 * 4; }   // [k step][piece][lane][4 dwords]

// ---- items: a constructor per form, and the dispatcher that reads the fields back ------------------------------------------
// PackItem's integer fields are named for the Winograd set; what another form keeps in them is written here and in pack_item's
// case for it, nowhere else.
static PackItem item(int kind, const float* w, void* out, int Cout, int Cin, int Cp = 0, int Np = 0, int dgrad = 0, int mode = 0) {
  return PackItem{w, (float*)out, Cout, Cin, Cp, Np, dgrad, 0u, kind, mode};
}
PackItem pack_wino(const float* w, float* U, int Cout, int Cin, int Cp, int dgrad, int prec) {
  return item(PACK_WINO, w, U, Cout, Cin, Cp, (Cout + 63) / 64 * 64, dgrad, prec);
}
PackItem pack_first_w(const float* w, float* wf, int Cout, int Cin) { return item(PACK_FIRST_W, w, wf, Cout, Cin); }
PackItem pack_first_mfma(const float* w, float* wfm, int Cout, int Cin) { return item(PACK_FIRST_MFMA, w, wfm, Cout, Cin); }
PackItem pack_convt_x3(const float* w, float* Wx, int Cin, int Cout, int dgrad) { return item(PACK_CONVT_X3, w, Wx, Cout, Cin, 0, 0, dgrad); }
PackItem pack_bias_tile(const float* bias, float* shift, int C, int reps) { return item(PACK_BIAS_TILE, bias, shift, C, reps); }
PackItem pack_dgrad_panel(const float* w, float* wp, int Cout, int Cin, int Cop, int KS, int Kp) {
  return item(PACK_DGRAD_PANEL, w, wp, Cout, Cin, Cop, Kp, KS);
}
PackItem pack_conv_panel(const float* w, void* wp, int dtype, int Cout, int Cin, int Cp, int KS, int Kp) {
  return item(PACK_CONV_PANEL, w, wp, Cout, Cin, Cp, Kp, KS, dtype);
}
PackItem pack_convt_panel(const float* w, void* wp, int dtype, int Cin, int Cout, int Kp) {
  return item(PACK_CONVT_PANEL, w, wp, Cout, Cin, 0, Kp, 0, dtype);
}
PackItem pack_convt_bf16f(const float* w, float* Wf, int Cin, int Cout) { return item(PACK_CONVT_BF16F, w, Wf, Cout, Cin); }
PackItem pack_convt_dgrad_panel(const float* w, float* wp, int Cin, int Cout, int Kp) {
  return item(PACK_CONVT_DGRAD_PANEL, w, wp, Cout, Cin, 0, Kp);
}

__device__ __forceinline__ void pack_item(const PackItem& t, unsigned vblock, unsigned vgrid) {
  switch (t.kind) {   // block-uniform
    case PACK_WINO: pack_wino_w_body(t.w, t.U, t.Cout, t.Cin, t.Cp, t.Np, t.dgrad, t.mode, vblock, vgrid); break;
    case PACK_FIRST_W: pack_first_w_body(t.w, t.U, t.Cout, t.Cin, vblock, vgrid); break;
    case PACK_FIRST_MFMA: pack_first_mfma_body(t.w, reinterpret_cast<uint16_t*>(t.U), t.Cout, t.Cin, vblock, vgrid); break;
    case PACK_CONVT_X3: pack_convt_x3_body(t.w, reinterpret_cast<uint16_t*>(t.U), t.Cin, t.Cout, t.dgrad, vblock, vgrid); break;
    case PACK_BIAS_TILE: pack_bias_tile_body(t.w, t.U, t.Cout, t.Cin, vblock, vgrid); break;
    case PACK_DGRAD_PANEL: pack_dgrad_w_body(t.w, t.U, t.Cout, t.Cin, t.Cp, t.dgrad, t.Np, vblock, vgrid); break;
    case PACK_CONV_PANEL:
      if (t.mode == 0) pack_conv_w_body(t.w, t.U, t.Cout, t.Cin, t.Cp, t.dgrad, t.Np, vblock, vgrid);
      else pack_conv_w_body(t.w, reinterpret_cast<__bf16*>(t.U), t.Cout, t.Cin, t.Cp, t.dgrad, t.Np, vblock, vgrid);
      break;
    case PACK_CONVT_PANEL:
      if (t.mode == 0) pack_convt_w_body(t.w, t.U, t.Cin, t.Cout, t.Np, vblock, vgrid);
      else pack_convt_w_body(t.w, reinterpret_cast<__bf16*>(t.U), t.Cin, t.Cout, t.Np, vblock, vgrid);
      break;
    case PACK_CONVT_BF16F: pack_convt_bf16f_body(t.w, reinterpret_cast<__bf16*>(t.U), t.Cin, t.Cout, vblock, vgrid); break;
    case PACK_CONVT_DGRAD_PANEL: pack_convt_dgrad_w_body(t.w, t.U, t.Cin, t.Cout, t.Np, vblock, vgrid); break;
    default: break;
  }
}

// workgroups an item runs on (256 threads, grid stride); 0: the item's shape does not fit its form
static unsigned pack_item_blocks(const PackItem& t) {
  int64_t work;   // threads' worth of elements
  switch (t.kind) {
    case PACK_WINO:
      if ((t.mode != 0 && t.mode != 1) || (t.Cp & (t.mode ? 15 : 7))) return 0;
      work = (int64_t)t.Np * t.Cp / (t.mode ? 8 : 1);
      break;
    case PACK_FIRST_W: work = 9 * 4 * (int64_t)t.Cout; break;
    case PACK_FIRST_MFMA: work = 2 * 64 * 8; break;
    case PACK_CONVT_X3:
      if ((t.Cin & (t.dgrad ? 63 : 15)) || (t.Cout & 31)) return 0;
      work = (int64_t)t.Cin * t.Cout * 4;
      break;
    case PACK_BIAS_TILE: work = (int64_t)t.Cout * t.Cin; break;
    case PACK_DGRAD_PANEL: work = (int64_t)t.Cin * t.Np; break;
    case PACK_CONV_PANEL: work = (int64_t)t.Cout * t.Np; break;
    case PACK_CONVT_PANEL: work = (int64_t)4 * t.Cout * t.Np; break;
    case PACK_CONVT_BF16F:
      if ((t.Cin & 63) || (t.Cout & 31)) return 0;
      work = (int64_t)t.Cin * t.Cout * 4;
      break;
    case PACK_CONVT_DGRAD_PANEL: work = (int64_t)t.Cin * t.Np; break;
    default: return 0;
  }
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(2048, (work + 255) / 256));
}

// ---- kernels and launchers --------------------------------------------------------------------------------------------------
// Every item of a table in ONE launch (a train step re-packs 17 forward + 17 data-gradient Winograd sets and the small forms after
// each optimizer step: launches of ~5 us, most of them smaller than a launch gap).  The table lives in device memory (the caller
// uploads it when it changes: a 1.6 KB by-value kernel argument cost ~100 us of host time per launch).
__global__ void pack_batch_kernel(const PackBatch* __restrict__ bp) {
  const PackBatch& b = *bp;
  int i = 0;
  while (i + 1 < b.n && blockIdx.x >= b.it[i + 1].blk0) ++i;   // <= PACK_MAX items: a linear scan of the block prefix
  const PackItem& t = b.it[i];
  pack_item(t, blockIdx.x - t.blk0, (i + 1 < b.n ? b.it[i + 1].blk0 : b.total_blocks) - t.blk0);
}

__global__ void pack_one_kernel(const PackItem it) { pack_item(it, blockIdx.x, gridDim.x); }

bool pack_batch_prepare(PackBatch& b) {
  unsigned blk = 0;
  for (int i = 0; i < b.n; ++i) {
    const unsigned blocks = pack_item_blocks(b.it[i]);
    if (!blocks) return false;
    b.it[i].blk0 = blk;
    blk += blocks;
  }
  b.total_blocks = blk;
  return true;
}

hipError_t launch_pack_batch(const PackBatch* batch_dev, unsigned total_blocks, hipStream_t s) {
  if (total_blocks == 0) return hipSuccess;
  hipLaunchKernelGGL(pack_batch_kernel, dim3(total_blocks), dim3(256), 0, s, batch_dev);
  return hipGetLastError();
}

hipError_t launch_pack_one(const PackItem& it, hipStream_t s) {
  const unsigned blocks = pack_item_blocks(it);
  if (!blocks) return hipErrorInvalidValue;
  hipLaunchKernelGGL(pack_one_kernel, dim3(blocks), dim3(256), 0, s, it);
  return hipGetLastError();
}

}  // namespace mgu
