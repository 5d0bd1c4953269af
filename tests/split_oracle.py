"""numpy restatement of the three-piece bf16 product of the fp32 kernels (csrc/device.h: split3_pack; csrc/pack.hip: the weight
packs), shared by tests/test_split_host.py (CPU) and tests/test_gpu_split_kernels.py (GPU).

An fp32 operand is cut into three bf16 pieces by TRUNCATION, a = p0 + p1 + p2 exactly, and a kernel keeps six of the nine piece
products: a0 b0, a0 b1, a1 b0, a0 b2, a1 b1, a2 b0 (SIX).  piece_gemm evaluates any subset of them with exact piece products and fp32
accumulation once per 16-wide k step and piece pair -- what v_mfma_f32_32x32x16_bf16 does up to its internal summation order -- so a
kernel that loses a product can be emulated without building one: MUTANTS.  The Winograd kernels run their 16 transform-domain GEMMs
that way between fp32 transforms; wino_fwd / wino_wgrad restate F(2x2,3x3) and F(3x3,2x2) with the standard matrices, and with
kept=None they are plain fp32 Winograd, the yardstick for those families (the transforms cost roundings a direct convolution does
not have).

Every error is measured in units of sum |a b| (err_units): the same operation on absolute values in float64, the natural scale of an
fp32 product sum.  A family (FAMILY) states one kernel family's operation three ways on the same operands: emulate (piece arithmetic),
ref64 (float64 result and scale) and, in the test modules, the fp32 CPU run and the GPU run."""
import numpy as np

F32, F64 = np.float32, np.float64


# ---- the split and the piece product ----------------------------------------------------------------------------------------------
def _trunc(a):
    return (a.view(np.uint32) & np.uint32(0xffff0000)).view(F32)


def split3(a):
    """The truncating three-way bf16 split of device.h: p0 = high half of a, p1 = high half of a - p0, p2 = high half of the rest."""
    a = np.ascontiguousarray(a, dtype=F32)
    p0 = _trunc(a)
    r1 = a - p0
    p1 = _trunc(r1)
    r2 = r1 - p1
    p2 = _trunc(r2)
    assert np.array_equal(p0.astype(F64) + p1.astype(F64) + p2.astype(F64), a.astype(F64)), "the split is exact"
    return p0, p1, p2


ORDER = ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))      # the kernels' issue order: smallest products first
SIX = frozenset(ORDER)
MUTANTS = {f"drop_a{i}b{j}": SIX - {(i, j)} for i, j in ORDER}
MUTANTS.update({
    "two_pieces": frozenset({(0, 0), (0, 1), (1, 0), (1, 1)}),          # two pieces per operand
    "three_products": frozenset({(0, 0), (0, 1), (1, 0)}),
    "a2_zero": frozenset(p for p in SIX if p[0] != 2),                  # a pack that leaves the third piece of A (B) zero
    "b2_zero": frozenset(p for p in SIX if p[1] != 2),
})
ALL_MUTANTS = tuple(MUTANTS)


def piece_gemm(A, B, kept=SIX):
    """A (..., M, K) @ B (..., K, N) in float32 out of the piece pairs `kept`; kept=None: a plain float32 matmul."""
    A, B = np.ascontiguousarray(A, dtype=F32), np.ascontiguousarray(B, dtype=F32)
    if kept is None:
        return np.matmul(A, B)
    pa, pb = [p.astype(F64) for p in split3(A)], [p.astype(F64) for p in split3(B)]
    acc = np.zeros(A.shape[:-1] + (B.shape[-1],), F32)
    for k0 in range(0, A.shape[-1], 16):
        for i, j in ORDER:
            if (i, j) in kept:   # a sum of 16 products of 8-bit significands: float64 holds it exactly unless exponents differ by > 30
                acc = (acc.astype(F64) + np.matmul(pa[i][..., k0:k0 + 16], pb[j][..., k0:k0 + 16, :])).astype(F32)
    return acc


def err_units(got, ref64, scale64):
    """max |got - ref| / sum |a b|; an output whose scale is zero must be exact."""
    err = np.abs(np.asarray(got, dtype=F64) - ref64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(scale64 > 0, err / scale64, np.where(err == 0, 0.0, np.inf))
    return float(q.max())


def passes(got, ref64, scale64, bar):
    """The predicate of the GPU tests (and of the host test that shows it rejects every designated mutant)."""
    return err_units(got, ref64, scale64) <= bar


# ---- operand builders -------------------------------------------------------------------------------------------------------------
def _rng(seed, tag):
    return np.random.default_rng([seed, sum(tag.encode())])


def _normal(rng, shape):
    return rng.standard_normal(shape).astype(F32)


def _bits(a, or_mask):
    return (np.ascontiguousarray(a, dtype=F32).view(np.uint32) | np.uint32(or_mask)).view(F32)


def _along(n, axis, ndim, v):
    s = [1] * ndim
    s[axis] = n
    return np.asarray(v, dtype=F32).reshape(s)


def _halves(a, axis):
    h = a.shape[axis] // 2
    lo, hi = [slice(None)] * a.ndim, [slice(None)] * a.ndim
    lo[axis], hi[axis] = slice(0, h), slice(h, 2 * h)
    return tuple(lo), tuple(hi)


def operands(case, shape_a, shape_b, red_a, red_b, seed, b_scale=0.125):
    """The two float32 operands of a product sum for operand case `case`; red_a / red_b: the axis of a / b the sum runs over (the
    per-position constructions follow it).  b is scaled by a power of two (weights are smaller than activations; bits unchanged)."""
    rng = _rng(seed, case)
    a, b = _normal(rng, shape_a), _normal(rng, shape_b)
    if case == "normal":                      # the suite's usual data
        pass
    elif case == "positive_low_bits":         # every lost term has the same sign: a mutant's bias cannot average out
        a, b = _bits(np.abs(a), 0xff), _bits(np.abs(b), 0xff)
    elif case == "full_mantissa":             # mantissa bits 15 and 0 set: the residual after the first piece spans 16 bits
        a, b = _bits(a, 0x8001), _bits(b, 0x8001)
        assert all(np.all(split3(v)[2] != 0) for v in (a, b)), "every third piece is nonzero"
    elif case == "cancellation":              # +v against -v (1 + 2^-12) under equal weights: the sum cancels to 2^-12 of its terms
        lo, hi = _halves(a, red_a)
        a[hi] = -a[lo] * F32(1 + 2.0 ** -12)
        lo, hi = _halves(b, red_b)
        b[hi] = b[lo]
    elif case == "wide_exponents":            # 2^e on a, 2^-e on b along the reduction, |e| <= 60
        e = np.round(np.linspace(-60, 60, shape_a[red_a]))
        assert shape_b[red_b] == shape_a[red_a]
        a = a * _along(len(e), red_a, a.ndim, 2.0 ** e)
        b = b * _along(len(e), red_b, b.ndim, 2.0 ** -e)
    elif case == "bf16_exact":                # second and third pieces are zero
        a, b = _trunc(a), _trunc(b)
    elif case == "integers":                  # exact in every piece, every transform and every sum
        return rng.integers(-3, 4, shape_a).astype(F32), rng.integers(-2, 3, shape_b).astype(F32)
    else:
        raise KeyError(case)
    return np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b * F32(b_scale), dtype=F32)


CASES = ("normal", "positive_low_bits", "full_mantissa", "cancellation", "wide_exponents", "bf16_exact", "integers")


# ---- float64 direct forms ---------------------------------------------------------------------------------------------------------
def conv3x3(x, w):
    """out[b,o,y,x] = sum x[b,c,y+r-1,x+s-1] w[o,c,r,s] in the dtype of the operands (float64 for a reference)."""
    B, C, H, W = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    out = np.zeros((B, w.shape[0], H, W), x.dtype)
    for r in range(3):
        for s in range(3):
            out += np.einsum("bchw,oc->bohw", xp[:, :, r:r + H, s:s + W], w[:, :, r, s])
    return out


def wgrad3x3(x, dz):
    """dw[o,c,r,s] = sum dz[b,o,y,x] x[b,c,y+r-1,x+s-1]."""
    B, C, H, W = x.shape
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)))
    dw = np.zeros((dz.shape[1], C, 3, 3), x.dtype)
    for r in range(3):
        for s in range(3):
            dw[:, :, r, s] = np.einsum("bohw,bchw->oc", dz, xp[:, :, r:r + H, s:s + W])
    return dw


def dgrad_weights(w):
    """The data gradient of a 3x3 / pad 1 convolution is the convolution of dz with w'[c][o][r][s] = w[o][c][2-r][2-s]."""
    return np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


# ---- Winograd in piece arithmetic -------------------------------------------------------------------------------------------------
def _take(a, axis, n):
    return [np.take(a, i, axis=axis) for i in range(n)]


def _bt(d, axis):      # B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]
    d0, d1, d2, d3 = _take(d, axis, 4)
    return np.stack([d0 - d2, d1 + d2, d2 - d1, d1 - d3], axis)


def _tiles(xp, th, tw, n):
    """t[..., ty, tx, i, j] = xp[..., 2 ty + i, 2 tx + j], i, j < n"""
    return np.stack([np.stack([xp[..., i:i + 2 * th:2, j:j + 2 * tw:2] for j in range(n)], -1) for i in range(n)], -2)


def wino_fwd(x, w, kept=SIX):
    """F(2x2,3x3) of x (B,C,H,W) with w (O,C,3,3), H and W even: fp32 transforms, the 16 GEMMs over C through piece_gemm."""
    x, w = np.asarray(x, dtype=F32), np.asarray(w, dtype=F32)
    B, C, H, W = x.shape
    O, th, tw = w.shape[0], H // 2, W // 2
    V = _bt(_bt(_tiles(np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1))), th, tw, 4), -2), -1)          # (B,C,th,tw,4,4)

    def g(a, axis):    # G = [1 0 0; 1/2 1/2 1/2; 1/2 -1/2 1/2; 0 0 1]
        g0, g1, g2 = _take(a, axis, 3)
        return np.stack([g0, ((g0 + g1) + g2) * F32(0.5), ((g0 - g1) + g2) * F32(0.5), g2], axis)

    U = g(g(w, -2), -1)                                                                             # (O,C,4,4)
    M = piece_gemm(V.transpose(4, 5, 0, 2, 3, 1).reshape(16, B * th * tw, C), U.transpose(2, 3, 1, 0).reshape(16, C, O), kept)
    M = M.reshape(4, 4, B, th, tw, O)

    def at(m, axis):   # A^T = [1 1 1 0; 0 1 -1 -1]
        m0, m1, m2, m3 = _take(m, axis, 4)
        return np.stack([(m0 + m1) + m2, (m1 - m2) - m3], axis)

    Y = at(at(M, 0), 1)                                                                             # (2,2,B,th,tw,O)
    return np.ascontiguousarray(Y.transpose(2, 5, 3, 0, 4, 1).reshape(B, O, H, W))


def wino_wgrad(x, dz, kept=SIX):
    """F(3x3,2x2) weight gradient of x (B,C,H,W), dz (B,O,H,W), H and W even: the 16 GEMMs run over the TILES."""
    x, dz = np.asarray(x, dtype=F32), np.asarray(dz, dtype=F32)
    B, C, H, W = x.shape
    O, th, tw = dz.shape[1], H // 2, W // 2
    V = _bt(_bt(_tiles(np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1))), th, tw, 4), -2), -1)          # (B,C,th,tw,4,4)

    def g(a, axis):    # G = [1 0; 1/2 1/2; 1/2 -1/2; 0 -1]
        z0, z1 = _take(a, axis, 2)
        return np.stack([z0, (z0 + z1) * F32(0.5), (z0 - z1) * F32(0.5), -z1], axis)

    S = g(g(_tiles(dz, th, tw, 2), -2), -1)                                                        # (B,O,th,tw,4,4)
    T = B * th * tw
    M = piece_gemm(S.transpose(4, 5, 1, 0, 2, 3).reshape(16, O, T), V.transpose(4, 5, 0, 2, 3, 1).reshape(16, T, C), kept)
    M = M.reshape(4, 4, O, C)

    def at(m, axis):   # A^T = [1 1 1 0; 0 1 -1 0; 0 1 1 1]
        m0, m1, m2, m3 = _take(m, axis, 4)
        return np.stack([(m0 + m1) + m2, m1 - m2, (m1 + m2) + m3], axis)

    return np.ascontiguousarray(at(at(M, 0), 1).transpose(2, 3, 0, 1))                              # (O,C,3,3)


# ---- the kernel families ----------------------------------------------------------------------------------------------------------
def elu64(v):
    v = np.asarray(v, dtype=F64)
    return np.where(v > 0, v, np.expm1(np.minimum(v, 0)))


class Family:
    """One kernel family's operation.  make(shape, case) -> operands (a, b); emulate(shape, a, b, kept) -> float32 result;
    ref64(shape, a, b) -> (float64 result, float64 scale = the operation on |a|, |b|).  Results are in the layout the reference
    framework uses for that operation (NCHW activations, OIHW weight gradients, (N, features) node tables)."""

    def post32(self, shape, pre):             # what follows the product sum in the kernel (activation, head mean)
        return pre

    def post64(self, shape, pre):
        return pre

    def scale64(self, shape, s):
        return s

    def ref64(self, shape, a, b):
        a, b = a.astype(F64), b.astype(F64)
        return self.post64(shape, self.direct(shape, a, b)), self.scale64(shape, self.direct(shape, np.abs(a), np.abs(b)))

    def emulate(self, shape, a, b, kept=SIX):
        return self.post32(shape, self.product(shape, a, b, kept))


class WinoFwd(Family):
    """Conv2d 3x3 / pad 1.  shape = (B, H, W, Cin, Cout); a = x (B,Cin,H,W), b = w (Cout,Cin,3,3)."""
    winograd = True

    def make(self, shape, case, seed=0):
        B, H, W, Ci, Co = shape
        return operands(case, (B, Ci, H, W), (Co, Ci, 3, 3), 1, 1, seed + Ci + Co)

    def direct(self, shape, a, b):
        return conv3x3(a, b)

    def product(self, shape, a, b, kept):
        return wino_fwd(a, b, kept)


class WinoDgrad(WinoFwd):
    """Its data gradient: a = dz (B,Cout,H,W), b = w (Cout,Cin,3,3); the same kernel on the flipped, transposed weights."""

    def make(self, shape, case, seed=0):
        B, H, W, Ci, Co = shape
        return operands(case, (B, Co, H, W), (Co, Ci, 3, 3), 1, 0, seed + Ci + Co + 1)

    def direct(self, shape, a, b):
        return conv3x3(a, dgrad_weights(b))

    def product(self, shape, a, b, kept):
        return wino_fwd(a, dgrad_weights(b), kept)


class WinoWgrad(Family):
    """Weight gradient of the same layer.  shape = (B, H, W, Cin, Cout); a = x (B,Cin,H,W), b = dz (B,Cout,H,W); the sum runs over
    the pixels (the constructions follow the W axis)."""
    winograd = True

    def make(self, shape, case, seed=0):
        B, H, W, Ci, Co = shape
        return operands(case, (B, Ci, H, W), (B, Co, H, W), 3, 3, seed + Ci + Co + 2, b_scale=1.0)

    def direct(self, shape, a, b):
        return wgrad3x3(a, b)

    def product(self, shape, a, b, kept):
        return wino_wgrad(a, b, kept)


class ConvT(Family):
    """ConvTranspose2d(2, stride 2), zero bias.  shape = (B, H, W, Cin, Cout); a = x (B,Cin,H,W), b = w (Cin,Cout,2,2).  One GEMM:
    rows = input pixels, k = ci, columns = (dy, dx, co)."""
    winograd = False

    def make(self, shape, case, seed=0):
        B, H, W, Ci, Co = shape
        return operands(case, (B, Ci, H, W), (Ci, Co, 2, 2), 1, 0, seed + Ci + Co + 3)

    def _gemm(self, shape, a, b, mm):
        B, H, W, Ci, Co = shape
        g = mm(a.transpose(0, 2, 3, 1).reshape(B * H * W, Ci), b.transpose(0, 2, 3, 1).reshape(Ci, 4 * Co))
        return np.ascontiguousarray(g.reshape(B, H, W, 2, 2, Co).transpose(0, 5, 1, 3, 2, 4).reshape(B, Co, 2 * H, 2 * W))

    def direct(self, shape, a, b):
        return self._gemm(shape, a, b, np.matmul)

    def product(self, shape, a, b, kept):
        return self._gemm(shape, a, b, lambda A, Bm: piece_gemm(A, Bm, kept))


class ConvTDgrad(Family):
    """Its data gradient.  a = dout (B,Cout,2H,2W), b = w (Cin,Cout,2,2); k = (qy, qx, co), K = 4 Cout."""
    winograd = False

    def make(self, shape, case, seed=0):
        B, H, W, Ci, Co = shape
        return operands(case, (B, Co, 2 * H, 2 * W), (Ci, Co, 2, 2), 1, 1, seed + Ci + Co + 4)

    def _gemm(self, shape, a, b, mm):
        B, H, W, Ci, Co = shape
        A = a.reshape(B, Co, H, 2, W, 2).transpose(0, 2, 4, 3, 5, 1).reshape(B * H * W, 4 * Co)
        g = mm(A, b.transpose(2, 3, 1, 0).reshape(4 * Co, Ci))
        return np.ascontiguousarray(g.reshape(B, H, W, Ci).transpose(0, 3, 1, 2))

    def direct(self, shape, a, b):
        return self._gemm(shape, a, b, np.matmul)

    def product(self, shape, a, b, kept):
        return self._gemm(shape, a, b, lambda A, Bm: piece_gemm(A, Bm, kept))


class FirstConv(Family):
    """relu(Conv2d(cin <= 3 -> 32, 3x3, pad 1)): K = 27 in the slot order of conv3x3_first_mfma_kernel -- k = 16 s + 8 h + e holds
    slot j = 8 s + e of lane half h = (tap 5 h + j // 3, channel j % 3), empty slots zero.  shape = (B, H, W, cin, layout); a = x
    (B,cin,H,W), b = w (32,cin,3,3).  The constructions follow the channel axis (with one channel they leave normal data)."""
    winograd = False

    def make(self, shape, case, seed=0):
        B, H, W, ci = shape[:4]
        return operands(case, (B, ci, H, W), (32, ci, 3, 3), 1, 1, seed + ci + 5)

    def _gemm(self, shape, a, b, mm):
        B, H, W, ci = shape[:4]
        xp = np.pad(a, ((0, 0), (0, 0), (1, 1), (1, 1)))
        A, Bm = np.zeros((B * H * W, 32), a.dtype), np.zeros((32, 32), a.dtype)
        for s in range(2):
            for h in range(2):
                for e in range(8):
                    j = 8 * s + e
                    tap, ch = 5 * h + j // 3, j % 3
                    if j < 15 and tap < 9 and ch < ci:
                        k, r, c = 16 * s + 8 * h + e, tap // 3, tap % 3
                        A[:, k] = xp[:, ch, r:r + H, c:c + W].reshape(-1)
                        Bm[k] = b[:, ch, r, c]
        return np.ascontiguousarray(mm(A, Bm).reshape(B, H, W, 32).transpose(0, 3, 1, 2))

    def direct(self, shape, a, b):
        return self._gemm(shape, a, b, np.matmul)

    def product(self, shape, a, b, kept):
        return self._gemm(shape, a, b, lambda A, Bm: piece_gemm(A, Bm, kept))

    def post32(self, shape, pre):
        return np.maximum(pre, F32(0))

    def post64(self, shape, pre):
        return np.maximum(pre, 0.0)


GAT_SHIFT = 7


class GatLinear(Family):
    """The linear layer of gat_fused2_kernel with the softmax out of the way: a ring in which node i hears node (i + 7) % N alone and
    zero attention vectors make every attention weight exactly 1, so out = ELU(X[src] W_h^T), heads concatenated or averaged.
    shape = (N, Fin, Fh, heads, concat); a = X (N,Fin), b = W (heads*Fh, Fin)."""
    winograd = False

    def make(self, shape, case, seed=0):
        N, Fin, Fh, heads, concat = shape
        return operands(case, (N, Fin), (heads * Fh, Fin), 1, 1, seed + Fin + Fh + heads + 6)

    @staticmethod
    def src(N):
        return (np.arange(N) + GAT_SHIFT) % N

    def direct(self, shape, a, b):
        return np.matmul(a[self.src(shape[0])], b.T)

    def product(self, shape, a, b, kept):
        return piece_gemm(a[self.src(shape[0])], b.T, kept)

    def post32(self, shape, pre):
        N, Fin, Fh, heads, concat = shape
        y = elu64(pre).astype(F32)
        if concat:
            return y
        t = y[:, :Fh].copy()
        for h in range(1, heads):
            t = t + y[:, h * Fh:(h + 1) * Fh]
        return t * F32(1.0 / heads)

    def post64(self, shape, pre):
        N, Fin, Fh, heads, concat = shape
        y = elu64(pre)
        return y if concat else y.reshape(N, heads, Fh).mean(1)

    def scale64(self, shape, s):
        N, Fin, Fh, heads, concat = shape
        return s if concat else s.reshape(N, heads, Fh).mean(1)


class GatAttention(GatLinear):
    """The same layer with the softmax in: three in-neighbours per node (i + 1, i + 7, i + 30) and nonzero attention vectors, on
    positive_low_bits features.  The kernel aggregates first, out = ELU((sum_j alpha_ij X_j) W_h^T): the attention weights are
    restated in the precision of the run (float32 for the emulation, float64 for the reference) and the product that follows goes
    through piece_gemm.  graph_attention.py:53-118: e = LeakyReLU(a_src . W x_j + a_tgt . W x_i), exp(e - max e), / (sum + 1e-10)."""
    SHIFTS = (1, 7, 30)

    def make(self, shape, case, seed=0):
        assert case == "positive_low_bits"
        return GatLinear.make(self, shape, case, seed + 1)

    def att(self, shape):
        N, Fin, Fh, heads, concat = shape
        return _rng(Fin + Fh + heads, "attention").uniform(-0.4, 0.4, (heads, 2 * Fh)).astype(F32)

    def edges(self, N):
        """(src, tgt) in CSR-by-target order"""
        tgt = np.repeat(np.arange(N), len(self.SHIFTS))
        return (tgt + np.tile(self.SHIFTS, N)) % N, tgt

    def _run(self, shape, X, W, dt, mm, alpha=0.2):
        N, Fin, Fh, heads, concat = shape
        src, tgt = self.edges(N)
        X, W, att = X.astype(dt), W.astype(dt), self.att(shape).astype(dt)
        pre, scale = [], []
        for h in range(heads):
            Wh = W[h * Fh:(h + 1) * Fh]
            hh = X @ Wh.T
            e = (hh @ att[h, :Fh])[src] + (hh @ att[h, Fh:])[tgt]
            e = np.where(e > 0, e, dt(alpha) * e)
            ex = np.exp(e - e.max())
            den = np.zeros(N, dt)
            np.add.at(den, tgt, ex)
            al = (ex / (den[tgt] + dt(1e-10))).astype(dt)
            agg, aggabs = np.zeros((N, Fin), dt), np.zeros((N, Fin), np.float64)
            for k in range(len(self.SHIFTS)):                       # a node's in-edges in order
                sl = slice(k, None, len(self.SHIFTS))
                agg = agg + al[sl, None] * X[src[sl]]
                aggabs = aggabs + np.abs(al[sl, None].astype(np.float64) * X[src[sl]])
            pre.append(mm(agg, Wh.T))
            scale.append(aggabs @ np.abs(Wh.T).astype(np.float64))
        return np.concatenate(pre, 1), np.concatenate(scale, 1)

    def ref64(self, shape, a, b):
        pre, scale = self._run(shape, a, b, F64, np.matmul)
        return self.post64(shape, pre), self.scale64(shape, scale)

    def emulate(self, shape, a, b, kept=SIX):
        return self.post32(shape, self._run(shape, a, b, F32, lambda A, Bm: piece_gemm(A, Bm, kept))[0])


FAMILY = {"wino_fwd": WinoFwd(), "wino_dgrad": WinoDgrad(), "wino_wgrad": WinoWgrad(), "convt_fwd": ConvT(), "convt_dgrad": ConvTDgrad(),
          "first_conv": FirstConv(), "gat_linear": GatLinear(), "gat_attention": GatAttention()}
