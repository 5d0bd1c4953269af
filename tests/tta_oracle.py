"""torch / float64 restatement of test-time augmentation's two kernels (csrc/tta.hip), written from their definitions and from none of
mgunet.tta's index arithmetic: the views through torch.flip / torch.rot90, the merge as the float64 mean of the views' softmaxes
mapped back, the error budget of the fp32 kernel, an fp32 numpy emulation of its operation order, and the seeded logits and view
tables that tests/test_tta_oracle_host.py (CPU) and tests/test_gpu_tta_kernels.py (device) share."""
import numpy as np
import torch

from mgunet import tta

# ---- views -------------------------------------------------------------------------------------------------------------------------


def view(x, flip, turns):
    """The view of (..., H, W): fW = torch.flip(x, (-1,)) for flip bit 0, fH = torch.flip(x, (-2,)) for bit 1, then
    torch.rot90(., turns, (-2, -1))."""
    if flip & 1:
        x = torch.flip(x, (-1,))
    if flip & 2:
        x = torch.flip(x, (-2,))
    return torch.rot90(x, turns, (-2, -1))


def unview(v, flip, turns):
    """The inverse of view: the quarter turns back, then the flips (each its own inverse)."""
    x = torch.rot90(v, -turns, (-2, -1))
    if flip & 2:
        x = torch.flip(x, (-2,))
    if flip & 1:
        x = torch.flip(x, (-1,))
    return x


# ---- merge -------------------------------------------------------------------------------------------------------------------------

def softmax64(logits):
    z = logits.double()
    e = torch.exp(z - z.amax(-1, keepdim=True))
    return e / e.sum(-1, keepdim=True)


def merge64(logits_by_group, table, B, C, H, W):
    """float64 (B, H, W, C): the mean over the rows (group, slot, flip, turns) of `table` of the softmax over C of that view's B
    images, logits_by_group[group][slot * B:(slot + 1) * B] of the (slots * B, Hg, Wg, C) float32 batch, mapped back with unview."""
    acc = torch.zeros((B, H, W, C), dtype=torch.float64)
    for g, slot, flip, turns in table:
        lg = logits_by_group[g][slot * B:(slot + 1) * B]
        assert lg.shape == ((B, W, H, C) if turns & 1 else (B, H, W, C)), (lg.shape, (g, slot, flip, turns))
        p = softmax64(lg).permute(0, 3, 1, 2)                       # (B, C, Hg, Wg)
        acc += unview(p, flip, turns).permute(0, 2, 3, 1)
    return acc / len(table)


def bound(C, K):
    """Absolute bound on |fp32 kernel - merge64| for probabilities <= 1, in units of 2^-24 (one fp32 rounding of a value <= 1):
      per view   the fp32 subtraction of the maximum moves the exponential by at most 0.37 (|d| 2^-24 exp(-|d|) <= 2^-24 / e);
                 expf costs up to 2 ulp; the sequential C-term sum has relative error (C - 1) 2^-24; the division is one rounding:
                 C + 3 in all, and the mean over the views keeps a per-view bound;
      merge      K additions on partial sums <= K before the 1/K scaling (K roundings after it), and one rounding for the scaling.
    (C + K + 4) 2^-24.  The merge term is that of a sequential fp32 sum; the kernel has since been changed to add the views in fp64 and
    round their mean once (a sequential fp32 sum of 8 equal softmaxes fl(1/3) or fl(1/5) misses 8 fl(1/C) by an ulp, which the
    all-equal case of the device tests caught), so its merge costs 1 of the K + 1 roundings allowed here; the bound is kept as derived.
    A numpy emulation of the kernel's order (emulate32 below) with sequential fp32 sums gave 1.1e-7 at C = 16, K = 8 against 1.67e-6
    and stayed under half the bound for C in {1, 2, 3, 4, 5, 8, 16}, K in {1, 2, 4, 8} and logit scales 0.5, 3 and 30; that measures
    the host's exp, not the device's expf (tests/test_gpu_tta_kernels.py records the device's figures)."""
    return (C + K + 4) * 2.0 ** -24


def emulate32(logits_by_group, table, B, C, H, W):
    """The kernel's operation order in numpy: per view, in float32, the maximum, the subtraction, np.exp, the left-to-right sum and
    the division; the views added in table order in float64 and multiplied by 1 / K there; one rounding to float32.  (B, H, W, C)."""
    acc = np.zeros((B, H, W, C), np.float64)
    for g, slot, flip, turns in table:
        lg = logits_by_group[g][slot * B:(slot + 1) * B].numpy()
        e = np.exp(lg - lg.max(-1, keepdims=True), dtype=np.float32)
        s = np.zeros(lg.shape[:-1], np.float32)
        for c in range(C):
            s = s + e[..., c]
        p = torch.from_numpy(e / s[..., None]).permute(0, 3, 1, 2)
        acc = acc + unview(p, flip, turns).permute(0, 2, 3, 1).numpy().astype(np.float64)
    return (acc * (1.0 / len(table))).astype(np.float32)


def margin(ref):
    """float64 (B, H, W): the gap between the two largest reference probabilities of each pixel (infinite for one class)"""
    if ref.shape[-1] == 1:
        return torch.full(ref.shape[:-1], float("inf"), dtype=torch.float64)
    top = ref.topk(2, dim=-1).values
    return top[..., 0] - top[..., 1]


# ---- view tables -------------------------------------------------------------------------------------------------------------------

NAMED = ("none", "hflip", "flips", "d4")
EXTRA = ("group1_only", "mixed_slots", "repeat")


def table(name, H, W):
    """the (group, slot, flip, turns) rows of a table: mgunet.tta.view_table's for the four named sets, else
      group1_only  K = 2, odd turns only (H != W): every view lies in group 1
      mixed_slots  K = 4, flips / turns (2,0), (1,1), (3,2), (0,3), the slots inside each group in reverse order of appearance
      repeat       K = 2, the view (2, 2) twice, in two slots holding different logits"""
    if name in NAMED:
        return [tuple(r) for r in tta.view_table(name, H, W)[0]]
    if name == "group1_only":
        assert H != W
        return [(1, 0, 3, 1), (1, 1, 2, 3)]
    if name == "repeat":
        return [(0, 0, 2, 2), (0, 1, 2, 2)]
    assert name == "mixed_slots"
    views = [(2, 0), (1, 1), (3, 2), (0, 3)]
    grp = [(r & 1) if H != W else 0 for _, r in views]
    left = [grp.count(0), grp.count(1)]
    rows = []
    for (f, r), g in zip(views, grp):
        left[g] -= 1
        rows.append((g, left[g], f, r))
    return rows


def group_shapes(rows, B, H, W):
    """[(images, Hg, Wg) or None] of the two shape groups' logits: (max slot + 1) * B images each"""
    slots = [0, 0]
    for g, slot, _, _ in rows:
        slots[g] = max(slots[g], slot + 1)
    return [(slots[0] * B, H, W) if slots[0] else None, (slots[1] * B, W, H) if slots[1] else None]


# ---- logits ------------------------------------------------------------------------------------------------------------------------

CASES = ("random", "spread", "huge", "dead", "equal", "tie_top", "one_hot")
DEAD = -1e30


def dead_classes(C):
    """every third class, starting at class 1 (a single class stays alive)"""
    return [c for c in range(C) if c % 3 == 1]


def tie_classes(C):
    assert C >= 3
    return 1, C - 1


def logits(case, shapes, C, seed):
    """float32 (images, Hg, Wg, C) per group of `shapes` (group_shapes), None for an empty group:
      random   N(0, 3^2)
      spread   classes alternate +60 / -60, plus N(0, 1): differences above 103, expf underflows to zero or a denormal
      huge     3e4 + N(0, 3^2), rounded to fp32 (the reference works from the rounded values)
      dead     N(0, 3^2) with dead_classes at -1e30: their probabilities are exactly 0
      equal    7.25 everywhere
      tie_top  random, but tie_classes both hold the pixel's maximum + 1 in every view
      one_hot  0 at an independently drawn class per view pixel, -200 elsewhere: the fp32 softmax is exactly one-hot"""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for shp in shapes:
        if shp is None:
            out.append(None)
            continue
        full = tuple(shp) + (C,)
        z = torch.randn(full, generator=gen, dtype=torch.float64)
        if case == "random":
            lg = 3.0 * z
        elif case == "spread":
            lg = z + (60.0 * (1 - 2 * (torch.arange(C) % 2))).double()
        elif case == "huge":
            lg = 3e4 + 3.0 * z
        elif case == "dead":
            lg = 3.0 * z
            for c in dead_classes(C):
                lg[..., c] = DEAD
        elif case == "equal":
            lg = torch.full(full, 7.25, dtype=torch.float64)
        elif case == "tie_top":
            a, b = tie_classes(C)
            lg = (3.0 * z).float()
            top = lg.amax(-1) + 1.0
            lg[..., a] = top
            lg[..., b] = top
        else:
            assert case == "one_hot"
            hot = torch.randint(0, C, tuple(shp), generator=gen)
            lg = (torch.nn.functional.one_hot(hot, C).double() - 1.0) * 200.0
        out.append(lg.float().contiguous())
    return out


# ---- the cases both test files run ---------------------------------------------------------------------------------------------------

SIZES = [(1, 1), (1, 19), (19, 1), (16, 16), (17, 31), (33, 16), (48, 64)]
MERGE_CLASSES = (1, 2, 3, 4, 5, 8, 16)
FLOAT_CASES = ("random", "spread", "huge", "dead")
# (table, (H, W), B): every named table at a square and a non-square size, the three extra tables, every size, B in {1, 3}
LAYOUTS = [
    ("none", (1, 1), 3), ("none", (1, 19), 1),
    ("hflip", (16, 16), 1), ("hflip", (19, 1), 3),
    ("flips", (16, 16), 3), ("flips", (17, 31), 1),
    ("d4", (16, 16), 3), ("d4", (33, 16), 3), ("d4", (48, 64), 1),
    ("group1_only", (17, 31), 3),
    ("mixed_slots", (16, 16), 1), ("mixed_slots", (33, 16), 1),
    ("repeat", (17, 31), 3),
]
EXACT_CLASSES = (1, 2, 3, 4, 5, 16)
# one table per K in {1, 2, 4, 8} on a square and on a non-square image, plus the group-1-only table
EXACT_LAYOUTS = [
    ("none", (16, 16), 3), ("none", (17, 31), 1),
    ("hflip", (1, 1), 1), ("hflip", (33, 16), 3),
    ("flips", (16, 16), 1), ("flips", (19, 1), 3),
    ("d4", (16, 16), 1), ("d4", (17, 31), 3), ("d4", (48, 64), 1),
    ("group1_only", (1, 19), 3), ("mixed_slots", (33, 16), 3),
]


def seed_of(case, C, name, H, W, B):
    return 1000 * CASES.index(case) + 50 * C + 7 * (NAMED + EXTRA).index(name) + 3 * H + W + B


def make(case, C, name, H, W, B):
    """(rows, per-group logits) of one case"""
    rows = table(name, H, W)
    return rows, logits(case, group_shapes(rows, B, H, W), C, seed_of(case, C, name, H, W, B))
