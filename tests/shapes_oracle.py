"""float64 numpy oracle of mgunet.object_shapes, shared by the shape tests and tools/make_shape_golden.py: the table of
include/mgunet.h (mgu_object_shapes) stated from an object's pixel coordinates -- centred coordinates, torch.cov's n - 1 covariance,
the per-pixel Mahalanobis terms of model/unet/shape_loss.py:161-176 -- and not from power sums, so it shares no route with the
kernel.

Conditioning.  float64 is enough while cov + eps I is well conditioned.  For a thin object -- at the limit a one-pixel-wide
diagonal line, whose covariance is singular -- the inverse has entries near 1 / eps and both np.linalg.inv and the per-pixel
products lose most of their digits.  The smaller eigenvalue is therefore always taken as det / l1 with the determinant from exact
Python integers (0 exactly for collinear pixels), and the term of an ill-conditioned object (l1 + eps > THIN_RATIO (l2 + eps)) is
evaluated in exact rational arithmetic (fractions.Fraction: the formula is a rational function of integers and eps) and rounded to
float64 once.  The reference itself is of no use there: it raises on the singular fp32 inverse or returns an eps-dominated value."""
from fractions import Fraction

import numpy as np

FIELDS = ("centroid", "cov", "axes", "angle", "fill", "term")


def too_large(n, w, h):
    """The exactness bound of mgu_object_moments: area * (max(w, h) - 1)^4 must stay below 2^64 (Python integers)."""
    return int(n) * (max(int(w), int(h)) - 1) ** 4 >= 2 ** 64


THIN_RATIO = 64.0          # (l1 + eps) / (l2 + eps) above which the term is evaluated exactly (the device switches routes at 256)
THIN_MAX_PIXELS = 20000    # the exact route is slow; larger thin objects stay in float64


def exact_term(ys, xs, eps):
    """mean_j (d_j^T (cov + eps I)^-1 d_j - 1)^2 in exact rational arithmetic, rounded to float64 once."""
    ys, xs = [int(v) for v in ys], [int(v) for v in xs]
    n, sx, sy = len(ys), sum(xs), sum(ys)
    a, b = [n * x - sx for x in xs], [n * y - sy for y in ys]                # n dx, n dy: integers
    n20, n11, n02 = sum(v * v for v in a) // n, sum(u * v for u, v in zip(a, b)) // n, sum(v * v for v in b) // n
    e = Fraction(eps)                                                        # cov = n20 / (n (n - 1)), d = (a, b) / n
    sxx, sxy, syy = Fraction(n20, n * (n - 1)) + e, Fraction(n11, n * (n - 1)), Fraction(n02, n * (n - 1)) + e
    det = sxx * syy - sxy * sxy
    tot = Fraction(0)
    for u, v in zip(a, b):
        m = (sxx * v * v - 2 * sxy * u * v + syy * u * u) / (det * n * n)
        tot += (m - 1) ** 2
    return float(tot / n)


def shape(ys, xs, epsilon=1e-6, min_pixels=10):
    """One object from its pixel coordinates: dict of float64 centroid [x, y], cov [c_xx, c_xy, c_yy], axes [a, b], angle, fill,
    term, the eigenvalues lam [l1, l2] and status (0 analysed, 1 fewer than min_pixels pixels, 2 past the exactness bound).  With
    status != 0 everything but the centroid is 0."""
    ys, xs = np.asarray(ys, np.float64), np.asarray(xs, np.float64)
    n = len(ys)
    out = {"centroid": np.array([xs.mean(), ys.mean()]), "cov": np.zeros(3), "axes": np.zeros(2), "angle": 0.0, "fill": 0.0,
           "term": 0.0, "lam": np.zeros(2), "status": 0}
    if n < max(min_pixels, 2):
        out["status"] = 1
        return out
    if too_large(n, xs.max() - xs.min() + 1, ys.max() - ys.min() + 1):
        out["status"] = 2
        return out
    dy, dx = ys - ys.mean(), xs - xs.mean()
    cxx, cxy, cyy = (dx * dx).sum() / (n - 1), (dx * dy).sum() / (n - 1), (dy * dy).sum() / (n - 1)
    cxy = cxy + 0.0                                                        # -0 -> +0
    rad = np.sqrt((0.5 * (cxx - cyy)) ** 2 + cxy ** 2)
    ix, iy = xs.astype(np.int64).tolist(), ys.astype(np.int64).tolist()
    sx, sy = sum(ix), sum(iy)
    n20, n02 = n * sum(v * v for v in ix) - sx * sx, n * sum(v * v for v in iy) - sy * sy
    n11 = n * sum(u * v for u, v in zip(ix, iy)) - sx * sy
    det = (n20 * n02 - n11 * n11) / (float(n) * (n - 1)) ** 2              # exact integer determinant: 0 for collinear pixels
    l1 = 0.5 * (cxx + cyy) + rad
    l2 = max(det, 0.0) / l1                                                # clamped at 0 before the square root
    a, b = 2.0 * np.sqrt(l1), 2.0 * np.sqrt(l2)
    eps = float(np.float32(epsilon))                                       # the reference's epsilon * eye(2) is a float32 tensor
    if l1 + eps > THIN_RATIO * (l2 + eps) and n <= THIN_MAX_PIXELS:
        term = exact_term(iy, ix, eps)
    else:
        inv = np.linalg.inv(np.array([[cyy + eps, cxy], [cxy, cxx + eps]]))    # (row, column) order, as torch.nonzero gives it
        d = np.stack([dy, dx], 1)
        term = float(np.mean((np.einsum("ni,ij,nj->n", d, inv, d) - 1.0) ** 2))
    out.update(cov=np.array([cxx, cxy, cyy]), axes=np.array([a, b]), angle=0.5 * np.arctan2(2.0 * cxy, cxx - cyy),
               fill=n / (np.pi * a * b) if b > 0 else 0.0, term=term, lam=np.array([l1, l2]))
    return out


def shapes_of_labels(labels, epsilon=1e-6, min_pixels=10):
    """shape() of objects 1..n of one labelled (H, W) map, in label order."""
    labels = np.asarray(labels)
    n = int(labels.max()) if labels.size else 0
    ys, xs = np.nonzero(labels)
    lab = labels[ys, xs]
    order = np.argsort(lab, kind="stable")
    ys, xs, lab = ys[order], xs[order], lab[order]
    cuts = np.searchsorted(lab, np.arange(1, n + 2))
    return [shape(ys[cuts[k]:cuts[k + 1]], xs[cuts[k]:cuts[k + 1]], epsilon, min_pixels) for k in range(n)]


def loss(shapes, keep=None):
    """Mean term of the analysed objects (those with keep[i] true, when given); 0.0 when there are none (shape_loss.py:180)."""
    t = [s["term"] for i, s in enumerate(shapes) if s["status"] == 0 and (keep is None or keep[i])]
    return float(np.mean(t)) if t else 0.0


def ulp32(v):
    """Spacing of float32 at |v|."""
    return float(np.spacing(np.float32(abs(v))))
