"""Host restatement of the bf16-storage forward, segment by segment, for tests/test_bf16_bars_host.py (CPU) and
tests/test_gpu_bf16_layers.py / tests/test_gpu_bf16.py / tests/test_gpu_bf16_convt.py (GPU).

segment() recomputes ONE exposed tensor of the bf16 forward from its exposed predecessors in float64 with the storage roundings of
oracle/mgunet_oracle.py (conv_block_bf16_storage, decoder_block_bf16_storage): bf16 weights (fp32 weights for a first convolution
on conv3x3_first_mfma_kernel / conv3x3_first_kernel: the three-piece weights of the former are the fp32 weights exactly), the folded
fp32 scale / shift, every stored activation rounded to bf16 (from the fp32 value a kernel holds), F.pad placement of the up-sampled
half.  Segments: skip0 <- input, skip_i <- pool(skip_i-1), feat_depth-1 <- skip_depth-1 (through the unexposed bottleneck),
feat_i <- feat_i+1, skip_i; the logits are the fp32 head on feat0.

The arithmetic of a segment is a table of five callables (Ops): conv3, convt, fold, store, place.  EXACT is the float64 reference;
EMULATIONS are CORRECT float32 evaluations that differ only in what a kernel is free to choose (channel-chunk order of 16 / 32 / 64,
tap-major against channel-major accumulation, fma against multiply-then-add in the fold); MUTANTS are emulated BROKEN kernels, each
a fault this code could really have (see the table below).  check() is the per-element bar:

  * mismatch share: on a shallow segment the fraction of elements with got != ref, on a deep one the fraction more than one bf16 ulp
    and one floor off (LIMITS, and the note there);
  * worst element in units of ulp_bf16(ref) + k * floor, at most 1, where floor_co = |scale_co| max|w_co| ulp_bf16(max|h|) is the
    absolute effect of a one-ulp flip of the unexposed layer h under the segment's last convolution on output channel co; a deep
    segment adds what two correct float32 evaluations differ from the float64 one on that channel (segment());
  * (kept from the older test) max-abs <= 1 % of the tensor's maximum; >= 90 % equal follows from the share on shallow segments and
    stays asserted on every segment of the older test's own shapes (tests/test_gpu_bf16.py).

Calibration (tests/test_bf16_bars_host.py prints and asserts it; figures of one run on the CPU, ragged size of every case):
  correct emulations (six float32 evaluation orders, every size), worst figure per case:
             shallow segments             deep segment
    case     mismatch %   coincidence k   mismatch %   beyond ulp + floor %   coincidence k
    f24d2    0.039        0.23            0.76         0.000                  0.65
    f40d2    0.132        0.71            1.36         0.000                  0.48
    f48d2    0.365        0.41            3.34         0.000                  0.63
    f96d1    0.025        0.21            1.82         0.000                  0.51
    f160d1   0.040        0.21            5.58         0.000                  0.52
    f32d2    0.146        0.21            2.31         0.004                  1.98
    f32d4    0.335        0.25            6.54         0.000                  0.62
    f32d1    0.022        0.10            0.25         0.000                  0.30
    f16d1    0.027        0.20            0.14         0.000                  0.30
    f64d1    0.058        0.22            1.36         0.000                  0.50
    limit    1.25         2               (none)       0.10                   3
  (the 8- and 16-feature cases of tests/test_gpu_bf16.py: at most 0.05 % and k 0.45 shallow, 0.002 % and k 1.30 deep; the oracle's
  float32 storage emulation run through the whole network and judged as the GPU tests judge: k <= 0.61 deep, but 13 - 19 % plain
  mismatches on the deep segment of f32d4, whose bottleneck is 3 x 4 or 4 x 6 pixels of 512 channels.)  Shallow: twice the worst
  mismatch share is 0.73 %, the worst coincidence plus one 1.71.  Deep (floor with the empirical term, see segment()): the worst
  coincidence plus one is 2.98; twice the worst share beyond ulp + floor is 0.008 %.
  mutants (ragged size of every case; every one that changes the arithmetic of a case fails on it):
    whole-image faults (lost k piece in a patch's last column / row, clamped bottom halo, swapped swizzle pieces, stale tap buffer,
    dropped N tail, exchanged ConvTranspose quadrants): 2 - 77 % mismatches and 65 - 2300 units on a shallow segment of every case;
    per-chunk bf16 partial sums / truncating store, everywhere: 14 - 49 % mismatches on a shallow segment; in edge patches only:
    1.65 - 44 % (the best mutant of the table: chunk_sums_bf16_edge on skip0 of f32d1, 1.3 x the limit; 1.4 - 15 x elsewhere);
    pad row written: 6.6 - 8.5 % mismatches on a shallow segment where one has an odd level (f32d2, f32d4); on the depth-2 cases at
    50 x 70 only the deep segment pads: 3.8 - 10.8 units and 0.4 - 3.9 % beyond ulp + floor (f48d2 the closest, 4.1 x the bar).
  Not applicable: n_tail_dropped where every N is a multiple of 32 (f96d1, f160d1, f32d*, f64d1); pad_row_written where no level is
  odd (the depth-1 cases).  No mutant is inapplicable everywhere.
  MI355X: no figures yet -- the GPU tests were written and calibrated on the CPU side and have not run on a GPU; each prints its
  figures per segment (pytest -s), which belong here beside the table.

Exact data (exact_params / exact_input): input in {0..3}; 3x3 weights in {-1, 0, +1} with NNZ nonzeros per output channel (half of
each sign) at positions of (tap, cin) given by a formula of (output channel, seed); BatchNorm gamma 1, beta 0, mean 0, variance 1
and zero convolution bias, so the folded shift is exactly 0 and the folded scale 1 / sqrt(1 + 1e-5) is absorbed by the bf16 store
of an integer below 256; two nonzeros per (cout, quadrant) and a small integer bias in the ConvTranspose; a dense {-1, 0, +1} fp32
head with integer bias.  Every stored value is a small integer, every partial sum exact in fp32 in any order: the network has
exactly one right answer, and unet_forward in float64 with eps = 1e-30 gives it."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import mgunet_oracle as O

F64 = torch.float64

# ---- the limits (calibrated by tests/test_bf16_bars_host.py, which asserts the conditions they have to meet) ----------------------
# A segment is DEEP when it runs through the unexposed bottleneck (feat_depth-1 <- skip_depth-1: five layers, up to 4600 terms per
# sum); every other segment is SHALLOW (two or three layers).  A one-ulp flip of an unexposed layer moves every output it feeds, and
# the outputs next to a rounding boundary or next to zero then differ: on a deep segment of a small image every output sees every
# flip, and the plain mismatch share of CORRECT float32 evaluations runs from 0 to 13 % (the older bar's 10 % rejects the CPU
# library's own order on f32d4 at 64 x 96).  The plain share is therefore the bar of shallow segments only; a deep segment is held by
# the share of elements more than one ulp AND one floor off, which the flips of a correct evaluation do not reach, and by the worst
# element.
LIMITS = {
    "shallow": {"mismatch": 0.0125, "beyond_floor": None, "k": 2.0},
    "deep": {"mismatch": None, "beyond_floor": 0.001, "k": 3.0},
}
MAX_REL_LIMIT = 1e-2        # the older bar, kept: max-abs <= 1 % of the tensor's maximum


def is_deep(depth, name):
    return name == f"feat{depth - 1}"


# ---- roundings --------------------------------------------------------------------------------------------------------------------
def bf16_rne(t):
    """Round to nearest even from the fp32 value a kernel holds (float64 -> fp32 -> bf16), back in t's dtype."""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


def bf16_trunc(t):
    f = t.to(torch.float32).contiguous()
    return (f.view(torch.int32) & -65536).view(torch.float32).to(t.dtype)


def ulp_bf16(t):
    """Spacing of bf16 at |t| (0 at 0), float64."""
    m, e = torch.frexp(t.to(F64).abs())
    return torch.where(m > 0, torch.ldexp(torch.ones_like(m), e - 8), torch.zeros_like(m))


def ulp_fp32(t):
    """Spacing of fp32 at |t| (0 at 0), float64."""
    m, e = torch.frexp(t.to(F64).abs())
    return torch.where(m > 0, torch.ldexp(torch.ones_like(m), e - 24), torch.zeros_like(m))


class Storage:
    """What a forward keeps its tensors in: the rounding of a stored weight, of a stored activation (from the fp32 value a kernel
    holds), and the spacing of the format.  BF16 is the bf16-storage forward; FP32 (tests/fp32_oracle.py) stores what it computes."""

    def __init__(self, name, weight, act, ulp):
        self.name, self.weight, self.act, self.ulp = name, weight, act, ulp


BF16 = Storage("bf16", O._bf16, bf16_rne, ulp_bf16)
FP32 = Storage("fp32", lambda w: w, lambda v: v, ulp_fp32)


# ---- geometry of the direct kernels (csrc/igemm.hip: launch_halo_tiles) -------------------------------------------------------------
def patch_rows(N):
    return 8 if N > 64 else 16          # the 128-channel tile walks 8 x 16 patches, the others 16 x 16


def n_tile(N):
    return 128 if N > 64 else 64 if N > 32 else 32


def edge_mask(H, W, TH):
    """Pixels of the patches that hang over the right / bottom image edge."""
    m = torch.zeros(H, W, dtype=torch.bool)
    if H % TH:
        m[H - H % TH:, :] = True
    if W % 16:
        m[:, W - W % 16:] = True
    return m


# ---- the arithmetic table ---------------------------------------------------------------------------------------------------------
class Ops:
    dtype = F64

    def __init__(self, name, **kw):
        self.name = name
        for k, v in kw.items():
            setattr(self, k, v)

    @staticmethod
    def conv3(x, w):
        return F.conv2d(x, w, padding=1)

    @staticmethod
    def convt(x, w, b):
        return F.conv_transpose2d(x, w, b, stride=2)

    @staticmethod
    def fold(z, scale, shift):
        return z * scale[None, :, None, None] + shift[None, :, None, None]

    @staticmethod
    def store(v):
        return bf16_rne(v)

    @staticmethod
    def pool(x):
        return F.max_pool2d(x, 2, 2)

    @staticmethod
    def place(up, H, W, bias):
        dy, dx = H - up.shape[2], W - up.shape[3]
        return F.pad(up, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])


EXACT = Ops("float64")


# ---- correct float32 emulations -----------------------------------------------------------------------------------------------------
def _emu_conv(chunk, per_tap):
    def conv3(x, w):
        C, H, W = x.shape[1], x.shape[2], x.shape[3]
        xp = F.pad(x, (1, 1, 1, 1))
        acc = torch.zeros(x.shape[0], w.shape[0], H, W, dtype=x.dtype)
        if chunk == 0:      # tap-major: all channels of one tap, then the next tap
            for t in range(9):
                dy, dx = divmod(t, 3)
                acc = acc + F.conv2d(xp[:, :, dy:dy + H, dx:dx + W], w[:, :, dy:dy + 1, dx:dx + 1])
            return acc
        for c0 in range(0, C, chunk):
            if per_tap:     # channel-chunk major, one tap at a time inside a chunk
                for t in range(9):
                    dy, dx = divmod(t, 3)
                    acc = acc + F.conv2d(xp[:, c0:c0 + chunk, dy:dy + H, dx:dx + W], w[:, c0:c0 + chunk, dy:dy + 1, dx:dx + 1])
            else:
                acc = acc + F.conv2d(x[:, c0:c0 + chunk], w[:, c0:c0 + chunk], padding=1)
        return acc
    return conv3


def _fold_fma(z, scale, shift):     # one rounding
    return (z.to(F64) * scale.to(F64)[None, :, None, None] + shift.to(F64)[None, :, None, None]).to(z.dtype)


EMULATIONS = {
    "library_order_muladd": Ops("library_order_muladd", dtype=torch.float32),       # whatever order the CPU library's float32 convolution has
    "chunk16_muladd": Ops("chunk16_muladd", dtype=torch.float32, conv3=_emu_conv(16, False)),
    "chunk32_fma": Ops("chunk32_fma", dtype=torch.float32, conv3=_emu_conv(32, False), fold=_fold_fma),
    "chunk64_muladd": Ops("chunk64_muladd", dtype=torch.float32, conv3=_emu_conv(64, False)),
    "tapmajor_fma": Ops("tapmajor_fma", dtype=torch.float32, conv3=_emu_conv(0, False), fold=_fold_fma),
    "chunk32_pertap_muladd": Ops("chunk32_pertap_muladd", dtype=torch.float32, conv3=_emu_conv(32, True)),
}


DEEP_FLOOR_FROM = ("library_order_muladd", "chunk32_pertap_muladd")


# ---- emulated broken kernels --------------------------------------------------------------------------------------------------------
def _tap_term(x, w, t, c0, c1):
    """Contribution of tap t, input channels c0:c1."""
    dy, dx = divmod(t, 3)
    H, W = x.shape[2], x.shape[3]
    xp = F.pad(x, (1, 1, 1, 1))
    return F.conv2d(xp[:, c0:c1, dy:dy + H, dx:dx + W], w[:, c0:c1, dy:dy + 1, dx:dx + 1])


def _lost_piece(where):
    def conv3(x, w):
        z = F.conv2d(x, w, padding=1)
        C, H, W = x.shape[1], x.shape[2], x.shape[3]
        if C < 8:
            return z
        TH = patch_rows(w.shape[0])
        lost = _tap_term(x, w, 5, C - 8, C)
        if where == "col":
            m = (torch.arange(W) % 16 == 15)[None, :].expand(H, W)
        else:
            m = (torch.arange(H) % TH == TH - 1)[:, None].expand(H, W)
        return z - lost * m
    return conv3


def _clamped_halo(x, w):
    H = x.shape[2]
    xp = F.pad(x, (1, 1, 1, 1))
    if H % patch_rows(w.shape[0]):
        xp[:, :, -1, :] = xp[:, :, -2, :]
    return F.conv2d(xp, w)


def _swizzle_swap(x, w):
    C = x.shape[1]
    if C < 16:
        return F.conv2d(x, w, padding=1)
    w = w.clone()
    rows = ((torch.arange(w.shape[0]) % n_tile(w.shape[0])) >> 1) & 7
    odd = (rows & 1) == 1
    a, b = w[odd, 0:8].clone(), w[odd, 8:16].clone()
    w[odd, 0:8], w[odd, 8:16] = b, a
    return F.conv2d(x, w, padding=1)


def _stale_tap(x, w):
    if x.shape[1] < 8:
        return F.conv2d(x, w, padding=1)
    w = w.clone()
    n1 = min(n_tile(w.shape[0]), w.shape[0])
    w[:n1, :, 1, 2] = w[:n1, :, 1, 1]          # tap 5 of N tile 0 reads the buffer tap 4 was staged in
    return F.conv2d(x, w, padding=1)


def _drop_n_tail(x, w):
    z = F.conv2d(x, w, padding=1)
    if x.shape[1] >= 8:
        z[:, 32 * (w.shape[0] // 32):] = 0
    return z


def _chunk_rounded(edge_only):
    def conv3(x, w):
        C, H, W = x.shape[1], x.shape[2], x.shape[3]
        if C < 8:
            return F.conv2d(x, w, padding=1)
        chunk = 64 if C % 64 == 0 else 32
        acc = torch.zeros(x.shape[0], w.shape[0], H, W, dtype=x.dtype)
        for c0 in range(0, C, chunk):
            acc = bf16_rne(acc + F.conv2d(x[:, c0:c0 + chunk], w[:, c0:c0 + chunk], padding=1))
        if edge_only:
            return torch.where(edge_mask(H, W, patch_rows(w.shape[0])), acc, F.conv2d(x, w, padding=1))
        return acc
    return conv3


def _store_trunc(edge_only):
    def store(v):
        if edge_only:
            return torch.where(edge_mask(v.shape[2], v.shape[3], patch_rows(v.shape[1])), bf16_trunc(v), bf16_rne(v))
        return bf16_trunc(v)
    return store


def _quadrant_swap(x, w, b):
    w = w.clone()
    w[:, :, 1, 0] = w[:, :, 0, 1]              # odd output rows read quadrant (dx, dy)
    return F.conv_transpose2d(x, w, b, stride=2)


def _pad_written(up, H, W, bias):
    dy, dx = H - up.shape[2], W - up.shape[3]
    out = bias[None, :, None, None].expand(up.shape[0], -1, H, W).clone()      # ConvTranspose of nothing: the (stored) bias
    out[:, :, dy // 2:dy // 2 + up.shape[2], dx // 2:dx // 2 + up.shape[3]] = up
    return out


MUTANTS = {
    "lost_piece_last_col": Ops("lost_piece_last_col", conv3=_lost_piece("col")),
    "lost_piece_last_row": Ops("lost_piece_last_row", conv3=_lost_piece("row")),
    "bottom_halo_clamped": Ops("bottom_halo_clamped", conv3=_clamped_halo),
    "swizzle_pieces_swapped": Ops("swizzle_pieces_swapped", conv3=_swizzle_swap),
    "stale_tap_buffer": Ops("stale_tap_buffer", conv3=_stale_tap),
    "n_tail_dropped": Ops("n_tail_dropped", conv3=_drop_n_tail),
    "chunk_sums_bf16": Ops("chunk_sums_bf16", conv3=_chunk_rounded(False)),
    "chunk_sums_bf16_edge": Ops("chunk_sums_bf16_edge", conv3=_chunk_rounded(True)),
    "store_truncates": Ops("store_truncates", store=_store_trunc(False)),
    "store_truncates_edge": Ops("store_truncates_edge", store=_store_trunc(True)),
    "convt_quadrants_swapped": Ops("convt_quadrants_swapped", convt=_quadrant_swap),
    "pad_row_written": Ops("pad_row_written", place=_pad_written),
}
# the faults of the index mapping (the others are faults of rounding: exact integer data cannot see them)
INDEXING = ("lost_piece_last_col", "lost_piece_last_row", "bottom_halo_clamped", "swizzle_pieces_swapped", "stale_tap_buffer",
            "n_tail_dropped", "convt_quadrants_swapped", "pad_row_written")


# ---- segments -----------------------------------------------------------------------------------------------------------------------
def _block(p, prefix, cur, first_fp32, ops, eps=1e-5, st=BF16):
    """ConvBlock with the storage roundings; returns (stored output, unit floor per output channel of the block's second conv)."""
    dt = ops.dtype
    floor = None
    for ci, (c, bn) in enumerate((("conv1", "bn1"), ("conv2", "bn2"))):
        w = p[prefix + c + ".weight"]
        if not (first_fp32 and ci == 0):
            w = st.weight(w)
        scale = p[prefix + bn + ".weight"] / torch.sqrt(p[prefix + bn + ".running_var"] + eps)            # fp32, as the library folds
        shift = p[prefix + bn + ".bias"] + (p[prefix + c + ".bias"] - p[prefix + bn + ".running_mean"]) * scale
        if ci == 1:
            hmax = cur.abs().max().to(F64)
            floor = scale.to(F64).abs() * w.to(F64).abs().amax(dim=(1, 2, 3)) * st.ulp(hmax)
        z = ops.conv3(cur.to(dt), w.to(dt))
        cur = ops.store(F.relu(ops.fold(z, scale.to(dt), shift.to(dt)))).to(dt)
    return cur, floor


def _decoder(p, bi, cur, skip, ops, eps=1e-5, st=BF16):
    pre = f"decoder.decoder_blocks.{bi}."
    dt = ops.dtype
    b = p[pre + "upsample.bias"].to(dt)
    up = st.act(ops.convt(cur.to(dt), st.weight(p[pre + "upsample.weight"]).to(dt), b))
    up = ops.place(up, skip.shape[2], skip.shape[3], st.act(b))
    return _block(p, pre + "conv_block.", torch.cat([skip.to(dt), up], dim=1), False, ops, eps, st)


def segment_names(depth):
    return [f"skip{i}" for i in range(depth)] + [f"feat{i}" for i in range(depth - 1, -1, -1)]


def segment(p, depth, name, src, first_fp32=False, ops=EXACT, st=BF16, eps=1e-5):
    """Exposed tensor `name` from its exposed predecessors `src` (a tuple: (x,) for skip0, (skip_i-1,) for skip_i, (skip_depth-1,)
    for feat_depth-1, (feat_i+1, skip_i) for feat_i), in ops' arithmetic.  Returns (tensor in float64, unit floor per channel)."""
    i = int(name[4:])
    with torch.no_grad():
        if name.startswith("skip"):
            cur = st.weight(src[0].to(torch.float32)) if i == 0 else ops.pool(src[0])
            out, fl = _block(p, f"encoder.encoder_blocks.{i}.", cur, first_fp32 and i == 0, ops, eps, st)
        elif i == depth - 1:
            bott, _ = _block(p, "encoder.bottleneck.", ops.pool(src[0]), False, ops, eps, st)
            out, fl = _decoder(p, 0, bott, src[0], ops, eps, st)
        else:
            out, fl = _decoder(p, depth - 1 - i, src[0], src[1], ops, eps, st)
    out = out.to(F64)
    if ops is EXACT and is_deep(depth, name):
        # four unexposed layers, not one: the floor of a deep segment is what two correct float32 evaluations are seen to differ from the
        # float64 one on this channel (the reference's own error), on top of the one-flip term
        for e in DEEP_FLOOR_FROM:
            fl = fl + (segment(p, depth, name, src, first_fp32, EMULATIONS[e])[0] - out).abs().amax(dim=(0, 2, 3))
    return out, fl


def sources(depth, name, x, sk, ft):
    i = int(name[4:])
    if name.startswith("skip"):
        return (x,) if i == 0 else (sk[i - 1],)
    return (sk[i],) if i == depth - 1 else (ft[i + 1], sk[i])


def chain(p, depth, x, first_fp32):
    """The float64 reference run through all segments on its own outputs: {name: (ref, floor, src)}."""
    sk, ft, out = {}, {}, {}
    for name in segment_names(depth):
        src = sources(depth, name, x, sk, ft)
        ref, fl = segment(p, depth, name, src, first_fp32)
        (sk if name.startswith("skip") else ft)[int(name[4:])] = ref
        out[name] = (ref, fl, src)
    return out


def first_fp32_weights(in_channels, init_features):
    """The first convolution keeps fp32 (three-piece) weights where conv3x3_first_mfma_kernel / conv3x3_first_kernel take it
    (csrc/elementwise.hip first_conv_applicable); elsewhere it is a bf16-weight layer of igemm_kernel<bf16>."""
    return in_channels <= 4 and init_features in (16, 32, 64)


# ---- the bar ------------------------------------------------------------------------------------------------------------------------
def measure(got, ref, floor, deep=False):
    got, ref = got.to(F64), ref.to(F64)
    err = (got - ref).abs()
    ulp = ulp_bf16(ref)
    fl = floor.to(F64)[None, :, None, None].expand_as(err)
    return {"mismatch": float((got != ref).double().mean()),                                   # share of elements that differ at all
            "beyond_ulp": float((err > ulp).double().mean()),                                  # ... by more than one bf16 ulp
            "beyond_floor": float((err > ulp + fl).double().mean()),                           # ... and one floor
            "worst": float((err / (ulp + LIMITS["deep" if deep else "shallow"]["k"] * fl)).max()),
            "k_needed": float(((err - ulp).clamp_min(0) / fl.clamp_min(1e-300)).max()),        # the k at which the worst element just passes
            "max_rel": float(err.max() / ref.abs().max().clamp_min(1e-30)), "finite": bool(torch.isfinite(got).all()), "deep": deep}


def failures(fig):
    """Which parts of the bar the figures miss (empty: passes)."""
    lim = LIMITS["deep" if fig["deep"] else "shallow"]
    out = []
    if not fig["finite"]:
        out.append("not finite")
    for share in ("mismatch", "beyond_floor"):
        if lim[share] is not None and fig[share] > lim[share]:
            out.append(share + " share")
    if fig["worst"] > 1.0:
        out.append("worst element")
    if fig["max_rel"] > MAX_REL_LIMIT:
        out.append("max-abs of max")
    return out


def passes(fig):
    return not failures(fig)


def check(got, ref, floor, tag="", deep=False):
    """The per-element bar; returns the figures it asserts."""
    fig = measure(got, ref, floor, deep)
    lim = LIMITS["deep" if deep else "shallow"]
    note = lambda key: f" (limit {lim[key]*100:.2f} %)" if lim[key] is not None else ""
    print(f"    [{tag}] {'deep' if deep else 'shallow'}: mismatch {fig['mismatch']*100:.4f} %{note('mismatch')}, beyond one ulp "
          f"{fig['beyond_ulp']*100:.4f} %, beyond one ulp and one floor {fig['beyond_floor']*100:.4f} %{note('beyond_floor')}, worst element "
          f"{fig['worst']:.3f} units of ulp + {lim['k']:g} floor (limit 1; k needed {fig['k_needed']:.2f}), max-abs {fig['max_rel']*100:.3f} % of max")
    assert not failures(fig), (tag, failures(fig), fig)
    return fig


# ---- exact data ---------------------------------------------------------------------------------------------------------------------
NNZ = 4             # nonzeros per output channel of a 3x3 convolution, half of each sign


def _stride(P):
    s = max(1, int(P * 0.618))
    while math.gcd(s, P) != 1:
        s += 1
    return s


def nnz_of(name, depth):
    """Four nonzeros let magnitudes grow by about a third per layer: past 255 in the 18 layers of a depth-4 network.  From depth 3 on
    the decoder's convolutions take two (+1, -1: a difference cannot exceed its operands) and values stay below 140."""
    return 2 if depth >= 3 and "decoder" in name else NNZ


def exact_seeds(cfg):
    """Seeds after which every (tap, cin) position of every 3x3 layer has been nonzero: nnz * cout * seeds >= 9 * cin, cin <= 2 cout."""
    return 9 if cfg[3] >= 3 else 5


def exact_params(cfg, seed):
    cin0, ncls, feats, depth = cfg
    p = O.make_unet_params(*cfg, seed=0)
    for name, v in p.items():
        if name.endswith("num_batches_tracked"):
            continue
        if name.endswith("conv1.weight") or name.endswith("conv2.weight"):
            cout, cin = v.shape[0], v.shape[1]
            P = 9 * cin
            S = _stride(P)
            w = torch.zeros(cout, P)
            co = torch.arange(cout)
            nnz = nnz_of(name, depth)
            for j in range(nnz):
                pos = ((co * nnz + j + seed * cout * nnz) * S) % P          # a bijection of the running index: no two coincide
                w[co, pos] = 1.0 if j % 2 == 0 else -1.0
            p[name] = w.reshape(cout, 9, cin).permute(0, 2, 1).reshape(cout, cin, 3, 3).contiguous()   # position = tap * cin + ci
        elif name.endswith("upsample.weight"):
            cin, cout = v.shape[0], v.shape[1]
            S = _stride(cin)
            w = torch.zeros(cin, cout, 2, 2)
            co = torch.arange(cout)
            for q in range(4):
                for j in range(2):
                    ci = ((co * 2 + j + 3 * seed + 5 * q) * S) % cin
                    w[ci, co, q // 2, q % 2] += 1.0 if j == 0 else -1.0
            p[name] = w
        elif name.endswith("upsample.bias"):
            p[name] = ((torch.arange(v.shape[0]) + seed) % 3).float()
        elif name.endswith("final_conv.weight"):
            k, ci = torch.meshgrid(torch.arange(v.shape[0]), torch.arange(v.shape[1]), indexing="ij")
            p[name] = (((ci * (k + 2) + seed) % 3) - 1).float().reshape(v.shape)
        elif name.endswith("final_conv.bias"):
            p[name] = (torch.arange(v.shape[0]) - 1 + seed % 2).float()
        elif name.endswith("running_var") or (".bn" in name and name.endswith(".weight")):
            p[name] = torch.ones_like(v)
        else:       # conv biases, BatchNorm beta and running mean: the folded shift is exactly zero
            p[name] = torch.zeros_like(v)
    return p


def exact_input(shape, seed):
    return torch.from_numpy(np.floor(O.formula_uniform("bf16exact/x", shape, 0.0, 4.0, seed)).clip(0, 3).astype(np.float32))


def exact_reference(p, x, depth):
    """The one right answer: the float64 network with the BatchNorm scale exactly 1."""
    with torch.no_grad():
        lg, sk, ft = O.unet_forward({k: (v.double() if v.dtype.is_floating_point else v) for k, v in p.items()}, x.double(), depth, eps=1e-30)
    return lg, sk, ft


# ---- the shape matrix ---------------------------------------------------------------------------------------------------------------
# case -> (cfg = (in_channels, classes, init_features, depth), the forms the case is there for: (form, Cin, Cout) of a layer it must
# contain).  Forms as layer_forms derives them from (Cp, N), the way halo_np / launch_halo_tiles / launch_tiles / convt_bf16f_layer do.
CASES = {
    "f24d2": ((3, 2, 24, 2), [("igemm", 24, 24), ("igemm", 48, 96), ("halo_np4_128tile", 96, 96), ("halo_np4_64tile", 96, 48),
                              ("convt_generic", 96, 48), ("convt_generic", 48, 24), ("igemm", 3, 24)]),
    "f40d2": ((3, 2, 40, 2), [("igemm", 40, 80), ("igemm", 80, 160), ("halo_np4_128tile", 160, 160), ("halo_np4_128tile", 160, 80),
                              ("convt_generic", 160, 80)]),
    "f48d2": ((3, 2, 48, 2), [("halo_np8_128tile", 192, 192), ("halo_np8_128tile", 192, 96), ("halo_np4_128tile", 96, 192),
                              ("convt_frag", 192, 96), ("convt_generic", 96, 48)]),
    "f96d1": ((3, 2, 96, 1), [("halo_np4_128tile", 96, 96), ("halo_np4_128tile", 96, 192), ("halo_np8_128tile", 192, 96),
                              ("convt_frag", 192, 96)]),
    "f160d1": ((3, 2, 160, 1), [("halo_np4_128tile", 160, 160), ("halo_np8_128tile", 320, 320), ("halo_np8_128tile", 320, 160),
                                ("convt_frag", 320, 160)]),
    "f32d2": ((1, 2, 32, 2), [("first_mfma", 1, 32), ("halo_np4_32tile", 32, 32), ("halo_np4_64tile", 32, 64),
                              ("halo_np8_128tile", 64, 128), ("halo_np8_32tile", 64, 32), ("convt_frag", 128, 64), ("convt_frag", 64, 32)]),
    "f32d4": ((3, 2, 32, 4), [("first_mfma", 3, 32), ("halo_np4_32tile", 32, 32), ("halo_np8_128tile", 512, 512),
                              ("halo_np8_64tile", 128, 64), ("convt_frag", 512, 256)]),
    "f32d1": ((3, 2, 32, 1), [("first_mfma", 3, 32), ("halo_np4_32tile", 32, 32), ("halo_np8_32tile", 64, 32), ("convt_frag", 64, 32)]),
    "f16d1": ((3, 2, 16, 1), [("first_valu", 3, 16), ("igemm", 16, 16), ("halo_np4_32tile", 32, 16), ("convt_generic", 32, 16)]),
    "f64d1": ((3, 2, 64, 1), [("first_valu", 3, 64), ("halo_np8_64tile", 64, 64), ("halo_np8_128tile", 64, 128),
                              ("halo_np8_64tile", 128, 64), ("convt_frag", 128, 64)]),
}
FAMILY = {"first_mfma": "conv3x3_first_mfma_kernel", "first_valu": "conv3x3_first_kernel", "igemm": "igemm_kernel<bf16>",
          "halo": "conv3x3_halo_kernel<bf16>", "convt_generic": "igemm_kernel<bf16> (ConvTranspose)", "convt_frag": "convt2x2_bf16_kernel"}


def layer_forms(cfg):
    """(form, Cin, Cout) of every convolution of the bf16 forward in launch order (the fp32 1x1 head is conv1x1_head_kernel)."""
    cin0, _, f, depth = cfg

    def conv(cin, cout, first=False):
        cp = -(-cin // 8) * 8
        if first and cp == 8 and cin <= 3 and cout == 32:
            return ("first_mfma", cin, cout)
        if first and cp == 8 and cin <= 4 and cout in (16, 32, 64):
            return ("first_valu", cin, cout)
        if cp % 32:
            return ("igemm", cin, cout)
        return (f"halo_np{8 if cp % 64 == 0 else 4}_{n_tile(cout)}tile", cin, cout)

    out, cin, c = [], cin0, f
    for i in range(depth):
        out += [conv(cin, c, first=i == 0), conv(c, c)]
        cin, c = c, 2 * c
    out += [conv(cin, c), conv(c, c)]
    for i in reversed(range(depth)):
        lo = f << i
        out += [("convt_frag" if (2 * lo) % 64 == 0 and lo % 32 == 0 else "convt_generic", 2 * lo, lo), conv(2 * lo, lo), conv(lo, lo)]
    return out


def family_launches(cfg):
    """Profiling-record name -> launches of one forward."""
    out = {}
    for form, _, _ in layer_forms(cfg):
        name = FAMILY["halo" if form.startswith("halo") else form]
        out[name] = out.get(name, 0) + 1
    return out
