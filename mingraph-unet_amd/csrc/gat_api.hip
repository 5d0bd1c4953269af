// GAT layer schedule behind the C-ABI (include/mgunet.h): replaces GraphAttentionLayer / MultiHeadGATLayer.forward
// (model/gat/graph_attention.py:40-118, 150-160), eval mode.  Host orchestration only; kernels in gat_fused.hip, gat.hip, igemm.hip.
//
// Launches per layer call with prepared weights (mgu_gat_prepare, once per weight version):
//   Fin <= F' (the patch GAT 32 -> 4 x 64, the stress graph 64 -> 4 x 64): gat_stmax (st + per-graph max) -> gat_fused  = 2
//   otherwise (a concat hidden layer):  GEMM [Wh | s | t] -> gat_edge_max -> gat_aggregate                              = 3
// No memset nodes: the per-(graph, head) max accumulators carry a generation number (gat_common.h), so stale words lose every max.
#include <algorithm>

#include "ctx.h"

using namespace mgu;
using namespace mgud;

struct mgu_gat_weights {
  int heads = 0, Fh = 0, Fin = 0;
  bool fused = false;
  float* buf = nullptr;   // fused: [wa (2H, Fin) | Wx (three bf16 pieces of W^T, fragment order)];  gather: packed panel (gat_pack_panel)
};

int mgud::gat_check_layer(mgu_ctx* c, const char* fn, int Fin, int heads, int Fh, bool train, int N) {
  if (heads < 1 || Fh < 4 || (Fh & 3) || Fin < 4 || (Fin & 3))
    return fail(c, MGU_ERR_INVALID, "%s needs Fin %% 4 == 0, Fout_head %% 4 == 0, heads >= 1 (Fin=%d Fout=%d heads=%d)", fn, Fin, Fh, heads);
  const int64_t HF = (int64_t)heads * Fh;
  if (!train && (heads > 32 || HF > 1024))
    return fail(c, MGU_ERR_INVALID, "%s supports heads <= 32 and heads * Fout_head <= 1024 (got %d x %d)", fn, heads, Fh);
  if (train && HF > 256) return fail(c, MGU_ERR_INVALID, "%s supports heads * Fout_head <= 256 (got %d x %d)", fn, heads, Fh);
  if (train && N * HF >= (1ll << 31)) return fail(c, MGU_ERR_INVALID, "%s: N * heads * Fout_head must be < 2^31", fn);
  return MGU_OK;
}

size_t mgud::gat_panel_floats(int heads, int Fh, int Fin) { return (size_t)rup(heads * Fh + 2 * heads, 128) * rup(Fin, 32); }

int mgud::gat_pack_panel(mgu_ctx* c, const float* W, const float* a, float* panel, int heads, int Fh, int Fin, bool clear, hipStream_t s) {
  // nn.Linear weight (F',Fin) stacked over heads is already the [N][K] panel (K padded to 32); rows HF.. hold
  // W^T a_src / W^T a_tgt so the same GEMM emits the attention scalars s, t (graph_attention.py:53,57-64)
  const int HF = heads * Fh, Kp = rup(Fin, 32);
  if (clear) HIPCHK(c, hipMemsetAsync(panel, 0, gat_panel_floats(heads, Fh, Fin) * sizeof(float), s));
  HIPCHK(c, launch_pack_one(pack_conv_panel(W, panel, 0, HF, Fin, Fin, 1, Kp), s));
  HIPCHK(c, launch_gat_wa_rows(W, a, panel, HF, heads, Fh, Fin, Kp, s));
  return MGU_OK;
}

// the call's graphs (no graph_ptr or num_graphs < 1: one graph, graph_ptr NULL), then their slotted per-(graph, head) max
// accumulators [64 slots][cap] of 64-bit (generation, value) words and this call's generation
int mgud::gmax_buffer(mgu_ctx* c, const int32_t** graph_ptr, int* num_graphs, int heads, unsigned long long** buf, unsigned* gen) {
  if (*num_graphs < 1 || !*graph_ptr) *num_graphs = 1, *graph_ptr = nullptr;
  const int need = *num_graphs * heads;
  if (need > c->gmax_cap) {
    const int cap = (std::max(need, 256) + 15) / 16 * 16;   // entries per slot: whole 128-byte lines
    if (c->gmaxbuf) {
      HIPCHK(c, hipDeviceSynchronize());
      HIPCHK(c, hipFree(c->gmaxbuf));
      c->gmaxbuf = nullptr;
    }
    HIPCHK(c, hipMalloc((void**)&c->gmaxbuf, (size_t)64 * cap * sizeof(unsigned long long)));
    HIPCHK(c, hipMemset(c->gmaxbuf, 0, (size_t)64 * cap * sizeof(unsigned long long)));
    c->gmax_cap = cap, c->gmax_gen = 0;
  }
  if (c->gmax_gen == 0xffffffffu) {   // generation wrap: start over from a cleared array
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemset(c->gmaxbuf, 0, (size_t)64 * c->gmax_cap * sizeof(unsigned long long)));
    c->gmax_gen = 0;
  }
  *buf = c->gmaxbuf;
  *gen = ++c->gmax_gen;
  return MGU_OK;
}

namespace {

// Prepares p for a layer shape (E_hint > 0: the graphs have edges) from W, a.  The allocation is kept while the shape and the
// schedule stay; a kept gather panel is repacked without clearing, its padding is still zero from the first fill.
int prepare_into(mgu_ctx* c, mgu_gat_weights* p, const float* W, const float* a, int heads, int Fh, int Fin, int64_t E_hint, hipStream_t s) {
  const bool fused = c->tn.gat_fused && gat_fused_applicable(Fin, heads, Fh, E_hint);
  const bool fresh = !p->buf || p->heads != heads || p->Fh != Fh || p->Fin != Fin || p->fused != fused;
  if (fresh) {
    if (p->buf) {
      HIPCHK(c, hipDeviceSynchronize());   // an earlier call may still read the old allocation
      (void)hipFree(p->buf);
      p->buf = nullptr;
    }
    p->heads = heads, p->Fh = Fh, p->Fin = Fin, p->fused = fused;
    const size_t bytes = (fused ? gat_fused_scratch_floats(Fin, heads, Fh) : gat_panel_floats(heads, Fh, Fin)) * sizeof(float);
    hipError_t e = hipMalloc((void**)&p->buf, bytes);
    if (e != hipSuccess) return fail(c, MGU_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  }
  if (!fused) return gat_pack_panel(c, W, a, p->buf, heads, Fh, Fin, fresh, s);
  HIPCHK(c, launch_gat_prep(W, a, p->buf, reinterpret_cast<unsigned*>(p->buf + (size_t)2 * heads * Fin), heads, Fh, Fin, s));
  return MGU_OK;
}

void free_weights(mgu_gat_weights* p) {
  if (p->buf) (void)hipFree(p->buf);
  delete p;
}

int forward_prepared(mgu_ctx* c, const mgu_gat_weights* p, const float* X, int N, const int32_t* rowptr, const int32_t* col, int64_t E,
                     const int32_t* graph_ptr, int num_graphs, int concat, float alpha, float* out, hipStream_t s) {
  const int heads = p->heads, Fh = p->Fh, Fin = p->Fin, HF = heads * Fh;
  unsigned long long* gmax;
  unsigned gen;
  int rc = gmax_buffer(c, &graph_ptr, &num_graphs, heads, &gmax, &gen);
  if (rc) return rc;
  Carve cv;
  if (p->fused && E > 0) {
    // aggregate-first path (gat_fused.hip): no (N, heads*F') node table, the gather moves Fin floats per edge
    const size_t o_st = cv.take((size_t)N * 2 * heads * 4);
    if ((rc = ensure(c, &c->gws, &c->gws_bytes, cv.off))) return rc;
    float* st = (float*)((char*)c->gws + o_st);
    int32_t* node_graph = nullptr;   // (no node -> graph table on this path: both kernels walk graph_ptr on the scalar unit)
    const float* wa = p->buf;
    const unsigned* wx = reinterpret_cast<const unsigned*>(p->buf + (size_t)2 * heads * Fin);
    {
      ProfScope ps(c, s, "gat_stmax_kernel");
      HIPCHK(c, launch_gat_stmax(X, wa, N, Fin, heads, rowptr, col, graph_ptr, num_graphs, alpha, st, node_graph, gmax, c->gmax_cap, gen, s));
    }
    ProfScope ps(c, s, "gat_fused2_kernel");
    HIPCHK(c, launch_gat_fused(X, Fin, st, rowptr, col, graph_ptr, num_graphs, gmax, wx, N, heads, Fh, concat, alpha, out, c->gmax_cap, gen, s));
    return MGU_OK;
  }
  // gather path: the prologue (Wh (N, HF) node table | st (N, 2H) attention scalars, per-graph max), then the row gather
  if (p->fused) return fail(c, MGU_ERR_STATE, "internal: aggregate-first weights on the gather path");
  const size_t o_wh = cv.take((size_t)N * HF * 4), o_st = cv.take((size_t)N * 2 * heads * 4), o_ng = cv.take((size_t)N * 4);
  if ((rc = ensure(c, &c->gws, &c->gws_bytes, cv.off))) return rc;
  char* g = (char*)c->gws;
  float *wh = (float*)(g + o_wh), *st = (float*)(g + o_st);
  int32_t* node_graph = num_graphs > 1 ? (int32_t*)(g + o_ng) : nullptr;   // node -> graph id (NULL: a single graph)
  if ((rc = gat_prologue(c, X, N, Fin, p->buf, heads, Fh, rowptr, col, E, graph_ptr, num_graphs, alpha, gmax, gen, wh, st, node_graph, nullptr,
                         true, s)))
    return rc;
  ProfScope ps(c, s, "gat_aggregate_kernel");
  HIPCHK(c, launch_gat_aggregate(wh, HF, st, rowptr, col, node_graph, gmax, N, E, heads, Fh, concat, alpha, out, c->gmax_cap, gen, s));
  return MGU_OK;
}

}  // namespace

extern "C" {

int mgu_gat_prepare(mgu_ctx* c, const void* W_dev, const void* a_dev, int heads, int Fout_head, int Fin, int has_edges,
                    mgu_gat_weights** out, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!W_dev || !a_dev || !out) return fail(c, MGU_ERR_INVALID, "NULL buffer");
  int rc = gat_check_layer(c, "mgu_gat_prepare", Fin, heads, Fout_head);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  mgu_gat_weights* p = new mgu_gat_weights();
  rc = prepare_into(c, p, (const float*)W_dev, (const float*)a_dev, heads, Fout_head, Fin, has_edges ? 1 : 0, (hipStream_t)hip_stream);
  if (rc) {
    free_weights(p);
    return rc;
  }
  *out = p;
  return MGU_OK;
}

void mgu_gat_release(mgu_ctx* c, mgu_gat_weights* p) {
  if (!p) return;
  if (c) (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  free_weights(p);
}

int mgu_gat_layer_forward_prepared(mgu_ctx* c, const mgu_gat_weights* p, const void* X_dev, int N, const int32_t* rowptr_dev,
                                   const int32_t* col_dev, int64_t E, const int32_t* graph_ptr_dev, int num_graphs, int concat, float alpha,
                                   void* out_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!p || N < 0 || E < 0) return fail(c, MGU_ERR_INVALID, "bad GAT arguments");
  if (N == 0) return MGU_OK;
  if (!X_dev || !rowptr_dev || !out_dev || (E > 0 && !col_dev)) return fail(c, MGU_ERR_INVALID, "NULL buffer");
  if (p->fused && E == 0) return fail(c, MGU_ERR_INVALID, "weights were prepared with has_edges = 1 but the graph has no edges");
  HIPCHK(c, hipSetDevice(c->device));
  return forward_prepared(c, p, (const float*)X_dev, N, rowptr_dev, col_dev, E, graph_ptr_dev, num_graphs, concat, alpha, (float*)out_dev,
                          (hipStream_t)hip_stream);
}

// One-shot form: prepares the weights on every call (one more launch), then runs the prepared schedule.
int mgu_gat_layer_forward(mgu_ctx* c, const void* X_dev, int N, int Fin, const int32_t* rowptr_dev, const int32_t* col_dev, int64_t E,
                          const int32_t* graph_ptr_dev, int num_graphs, const void* W_dev, const void* a_dev, int heads,
                          int Fout_head, int concat, float alpha, void* out_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (N < 0 || E < 0) return fail(c, MGU_ERR_INVALID, "bad GAT arguments");
  int rc = gat_check_layer(c, "mgu_gat_layer_forward", Fin, heads, Fout_head);
  if (rc) return rc;
  if (N == 0) return MGU_OK;
  if (!X_dev || !rowptr_dev || !W_dev || !a_dev || !out_dev || (E > 0 && !col_dev)) return fail(c, MGU_ERR_INVALID, "NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  if (!c->gat_tmp) c->gat_tmp = new mgu_gat_weights();
  if ((rc = prepare_into(c, c->gat_tmp, (const float*)W_dev, (const float*)a_dev, heads, Fout_head, Fin, E, s))) return rc;
  return forward_prepared(c, c->gat_tmp, (const float*)X_dev, N, rowptr_dev, col_dev, E, graph_ptr_dev, num_graphs, concat, alpha,
                          (float*)out_dev, s);
}

}  // extern "C"

void mgud::gat_destroy(mgu_ctx* c) {
  if (c->gat_tmp) free_weights(c->gat_tmp);
  c->gat_tmp = nullptr;
  if (c->gmaxbuf) (void)hipFree(c->gmaxbuf);
  c->gmaxbuf = nullptr;
}
