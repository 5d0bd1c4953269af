"""Guard against the next paste: each shared device / launch helper of csrc/ has ONE definition, and the kernel files declare no
vector typedefs of their own (csrc/device.h, common.h and ctx.h are where they live; objects_common.h for what only the object-level
kernel files share).  Source text only: no GPU, no build."""
import glob
import os
import re

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mingraph-unet_amd", "csrc")
SOURCES = {os.path.basename(p): open(p).read() for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))}

VECTOR_TYPES = ["f32x16", "f32x4", "f32x2", "u32x4", "u32x2", "bf16x8"]
DEVICE_HELPERS = ["mfma_bf16", "split3_pack", "split3_pack_s", "x3_add", "x3_sub", "x3_fma", "static_for", "lds_barrier",
                  "lds_barrier_builtin", "lds_barrier_fenced", "wave_sum", "wave_min", "wave_max", "block_fold", "enc_ordered",
                  "dec_ordered", "graph_of"]
HOST_HELPERS = ["grid_for", "aligned16", "rup", "ensure"]
# objects.hip, shapes.hip, split.hip, instances.hip: the wave group-by, the two scans, the pixel -> object rule (objects_common.h)
OBJECT_HELPERS = ["wave_by_key", "block_exclusive_scan", "chunk_sum_scan", "object_index", "objects_recorded"]
# names the private copies went by
RETIRED = ["f32x4c", "f32x4n", "f32x4r", "u32x4_t", "x3_static_for", "scalar_fma", "ww_barrier", "gat_enc_ordered", "gat_dec_ordered",
           "gf_enc_ordered", "gf_dec_ordered", "wave_sum64", "fold_doubles", "nblocks", "nblk", "nb", "al16", "align256", "LEADER_ROUNDS",
           "SH_ROUNDS"]


def definitions(name):
    """(file, line) of every function definition `name(...) {` or typedef / struct of that name"""
    func = re.compile(r"^[^\n;=(]*?[\w>&*]\s+" + name + r"\s*\([^;{}]*\)\s*(?:const\s*)?\{", re.M)   # declarator at the start of a line, body follows
    typ = re.compile(r"^\s*(?:typedef\b[^;]*\b" + name + r"\b[^;]*;|struct\s+" + name + r"\s*\{|using\s+" + name + r"\s*=)", re.M)
    return [(f, t.count("\n", 0, m.start()) + 1) for f, t in SOURCES.items() for m in list(func.finditer(t)) + list(typ.finditer(t))]


def test_each_shared_helper_is_defined_once():
    where = {n: definitions(n) for n in VECTOR_TYPES + DEVICE_HELPERS + HOST_HELPERS + ["Carve"]}
    assert {n: w for n, w in where.items() if len(w) != 1} == {}
    assert {n: w for n, w in where.items() if n in VECTOR_TYPES + DEVICE_HELPERS and w[0][0] != "device.h"} == {}
    assert {n: w for n, w in where.items() if n not in VECTOR_TYPES + DEVICE_HELPERS and w[0][0] not in ("common.h", "ctx.h")} == {}


def test_kernel_files_declare_no_vector_types_and_retired_names_are_gone():
    assert [f for f, t in SOURCES.items() if f.endswith(".hip") and "ext_vector_type" in t] == []
    assert {n: definitions(n) for n in RETIRED if definitions(n)} == {}
    assert [(f, n) for f, t in SOURCES.items() for n in RETIRED[:4] if re.search(r"\b" + n + r"\b", t)] == []


def test_object_helpers_live_in_objects_common_h_only():
    """one definition each, in objects_common.h; the private round counts of the wave group-by copies are gone (they were constants,
    so the text is searched), and no kernel file spells the group-by's loop or a Hillis-Steele scan of its own"""
    where = {n: definitions(n) for n in OBJECT_HELPERS}
    assert {n: w for n, w in where.items() if [f for f, _ in w] != ["objects_common.h"]} == {}
    assert [(f, n) for f, t in SOURCES.items() for n in RETIRED[-2:] if re.search(r"\b" + n + r"\b", t)] == []
    family = ["objects.hip", "shapes.hip", "split.hip", "instances.hip"]
    assert [f for f in family if '#include "objects_common.h"' not in SOURCES[f]] == []
    assert [f for f in family if re.search(r"for \([^)]*\) \{\s*const unsigned long long act = __ballot|SCAN_THREADS\s*=|sh\[tid - off\]", SOURCES[f])] == []


LOSS_FILES = ["losses.hip", "lovasz.hip", "pixel_ce.hip"]
LOSS_HELPERS = ["softmax_front", "NoClassHook", "LossCall", "LossTile", "loss_tile", "loss_item", "up_scale", "LossGrad", "loss_call", "with_nc", "with_flag",
                "int_c"]
RETIRED_LOSS = ["LvCall", "LvTile", "PcTile", "LvGrad", "PcGrad", "LV_ITEMS", "PC_ITEMS", "LV_TILE", "PC_TILE", "lv_tile", "pc_tile", "pc_item"]


def test_loss_helpers_live_in_loss_common_h_only():
    """the softmax front end, the call descriptor, the tile arithmetic, the gradient request, the shared host checks and the
    compile-time dispatch of the segmentation losses: one definition each, in loss_common.h, which the three kernel files include.
    Their private copies are gone, no macro selects a kernel, no file forms an exponential or maps the error word itself."""
    where = {n: definitions(n) for n in LOSS_HELPERS}
    assert {n: w for n, w in where.items() if [f for f, _ in w] != ["loss_common.h"]} == {}
    assert [f for f in LOSS_FILES if '#include "loss_common.h"' not in SOURCES[f]] == []
    assert [(f, n) for f, t in SOURCES.items() for n in RETIRED_LOSS if re.search(r"\b" + n + r"\b", t)] == []
    assert [f for f in LOSS_FILES if "#define MGU_" in SOURCES[f]] == []
    assert [f for f in LOSS_FILES if re.search(r"\bexpf\s*\(", SOURCES[f])] == []
    assert "hipHostMallocMapped" not in SOURCES["losses.hip"]
    assert len(re.findall(r"\bsoftmax_front\s*\(", "".join(SOURCES[f] for f in LOSS_FILES))) == 5


PACK_BODIES = ["pack_wino_w_body", "pack_first_w_body", "pack_first_mfma_body", "pack_convt_x3_body", "pack_bias_tile_body",
               "pack_dgrad_w_body", "pack_conv_w_body", "pack_convt_w_body", "pack_convt_bf16f_body", "pack_convt_dgrad_w_body"]


def test_weight_form_packers_live_in_pack_hip_only():
    """every element loop of a weight form and their dispatcher are defined once, in pack.hip, and no other kernel file launches a
    packer of its own (elementwise.hip keeps pack_input_kernel: activations, not weights)"""
    where = {n: definitions(n) for n in PACK_BODIES + ["pack_item"]}
    assert {n: w for n, w in where.items() if [f for f, _ in w] != ["pack.hip"]} == {}
    found = set(re.findall(r"\b(pack_\w+_body)\b", "".join(SOURCES.values())))
    assert found == set(PACK_BODIES)
    kernels = {f: re.findall(r"__global__\s[^;{(]*?\b(pack_\w*)\s*\(", t) for f, t in SOURCES.items() if f.endswith(".hip")}
    assert {f: k for f, k in kernels.items() if k and f != "pack.hip"} == {"elementwise.hip": ["pack_input_kernel"]}
    assert sorted(kernels["pack.hip"]) == ["pack_batch_kernel", "pack_one_kernel"]


HOST_CONV_FILES = ["mgunet_api.hip", "mgunet_train.hip", "bwd_blocks.hip"]
RETIRED_HOST = ["caller_layer", "block_layer", "last_stat_rows", "t_ldin", "t_ldy", "t_feat", "t_pooled", "t_logits"]


def test_layer_shapes_come_from_one_builder_and_launches_report_in_a_struct():
    """make_layer (ctx.h) is the only place that derives K, Kp, N, Np of a layer: the host files of the convolution path assign
    neither padded size themselves.  The private builders, the forward record kept inside Layer and the value handed back through
    the context are gone, and no function of ctx.h reports through a bool* out-parameter."""
    assert [f for f, _ in definitions("make_layer")] == ["ctx.h"]
    assert [(f, m.group(0)) for f in HOST_CONV_FILES for m in re.finditer(r"[.>](?:Kp|Np)\s*=(?!=)", SOURCES[f])] == []
    assert [(f, n) for f, t in SOURCES.items() for n in RETIRED_HOST if re.search(r"\b" + n + r"\b", t)] == []
    assert re.findall(r"\bbool\s*\*", SOURCES["ctx.h"]) == []
