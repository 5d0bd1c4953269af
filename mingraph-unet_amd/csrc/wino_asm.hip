// Host side of the hand-scheduled assembly form of the wide component-pair Winograd kernel (asm/gen_wino_cp.py emits the
// kernel, the Makefile assembles it into a gfx950 code object and embeds it in the library as a byte array).
//
// Same operator, same layouts and the same arithmetic order as wino3x3_cp_kernel<2, false, false, false> (wino_f32.hip; the
// 3x3 convolutions of ConvBlock, model/unet/unet_encoder.py:15-25): outputs are bitwise equal to the C++ kernel's
// (tests/test_gpu_wino_asm.py).  The code object is loaded once per device through the module API; everything the assembly
// does not cover (ragged sizes, statistics epilogue, odd chunk counts) stays on the C++ kernel (pick_conv, igemm.hip).
#include "common.h"
#include <cstddef>
#include <mutex>

extern "C" const unsigned char mgu_wino_cp2_hsaco[];
extern "C" const unsigned mgu_wino_cp2_hsaco_len;
extern "C" const unsigned char mgu_wino_cp1r2h_hsaco[];   // the head-fused form of the 2-chunk narrow kernel: a code object of its own
extern "C" const unsigned mgu_wino_cp1r2h_hsaco_len;

namespace mgu {

namespace {
struct WinoAsmArgs {          // kernarg segment of mgu_wino_cp2_gfx950 (asm/gen_wino_cp.py: emit_prologue)
  const float* in;            //   0
  const void* wu;             //   8
  float* out;                 //  16  d.out + d.coff
  const float* scale;         //  24
  const float* shift;         //  32
  float* pool;                //  40  may be null
  int H, W, ldin, ldout;      //  48
  int ldpool, nC, relu, tiles_x;      //  64
  int tiles_y, total, ppb, ngroups;   //  80
  int nitems, per_xcd;                //  96
  unsigned mg_ngroups, mg_tx;         // 104  floor(2^32 / d) (0xffffffff for d == 1)
  unsigned mg_txty, pad;              // 112
};
static_assert(sizeof(WinoAsmArgs) == 120, "kernarg layout of mgu_wino_cp2_gfx950");
struct WinoAsmHeadArgs {      // kernarg segment of mgu_wino_cp1r2h_gfx950 (emit_head_prologue): the plain block, then the head's
  WinoAsmArgs a;              //   0
  const float* head_w;        // 120
  const float* head_b;        // 128
  float* logits;              // 136
  float* psum;                // 144
  int ncls, psum_bytes;       // 152
};
static_assert(sizeof(WinoAsmHeadArgs) == 160 && offsetof(WinoAsmHeadArgs, head_w) == 120, "kernarg layout of mgu_wino_cp1r2h_gfx950");

unsigned magic(unsigned d) { return d <= 1 ? 0xffffffffu : (unsigned)((1ull << 32) / d); }

// the code object's kernels: the wide one and the narrow ones of 2 and 4 chunks (32 / 64 input channels)
// ... and the head-fused form of the first narrow one (module 1)
const char* const kNames[4] = {"mgu_wino_cp2_gfx950", "mgu_wino_cp1r2_gfx950", "mgu_wino_cp1r4_gfx950", "mgu_wino_cp1r2h_gfx950"};
std::mutex g_mu;
hipModule_t g_mod[64][2] = {};
hipFunction_t g_fn[64][4] = {};   // loaded functions per device (kNames order), written once under g_mu, immutable afterwards
}  // namespace

hipError_t launch_wino_cp_asm(const IgemmDesc& d, ConvKernel kind, hipStream_t s, const WinoHead* head) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
  hipFunction_t fn;
  const int k = kind == ConvKernel::WinoAsmWide ? 0 : kind == ConvKernel::WinoAsmCp1r2 ? 1 : kind == ConvKernel::WinoAsmCp1r4 ? 2 : 3;
  if ((k == 3) != (head != nullptr)) return hipErrorInvalidValue;
  const int m = k == 3 ? 1 : 0;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_mod[dev][m]) {
      e = hipModuleLoadData(&g_mod[dev][m], m ? mgu_wino_cp1r2h_hsaco : mgu_wino_cp2_hsaco);
      if (e != hipSuccess) return e;
    }
    if (!g_fn[dev][k]) {
      e = hipModuleGetFunction(&g_fn[dev][k], g_mod[dev][m], kNames[k]);
      if (e != hipSuccess) return e;
    }
    fn = g_fn[dev][k];
  }
  const WinoPlan p = wino_plan(d);
  WinoAsmHeadArgs ha;
  WinoAsmArgs& a = ha.a;
  a.in = d.in, a.wu = d.wu, a.out = d.out + d.coff, a.scale = d.scale, a.shift = d.shift, a.pool = d.pool;
  a.H = d.H, a.W = d.W, a.ldin = d.ldin, a.ldout = d.ldout;
  a.ldpool = d.pool ? d.ldpool : 0, a.nC = d.Cp >> 4, a.relu = d.relu, a.tiles_x = p.tiles_x;
  a.tiles_y = p.tiles_y, a.total = p.total, a.ppb = p.ppb, a.ngroups = p.ngroups;
  a.nitems = p.ngroups * p.nblk, a.per_xcd = p.per_xcd;
  a.mg_ngroups = magic((unsigned)p.ngroups), a.mg_tx = magic((unsigned)p.tiles_x);
  a.mg_txty = magic((unsigned)(p.tiles_x * p.tiles_y)), a.pad = 0;
  size_t sz = sizeof(a);
  if (head) {
    ha.head_w = head->w, ha.head_b = head->b, ha.logits = head->logits, ha.psum = head->psum;
    ha.ncls = head->ncls, ha.psum_bytes = head->psum_bytes;
    sz = sizeof(ha);
  }
  void* extra[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &ha, HIP_LAUNCH_PARAM_BUFFER_SIZE, &sz, HIP_LAUNCH_PARAM_END};
  return hipModuleLaunchKernel(fn, (unsigned)(8 * p.per_xcd), 1, 1, 512, 1, 1, 0, s, nullptr, extra);
}

}  // namespace mgu
