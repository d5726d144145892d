"""numpy model of the F+tree weighted sampler as include/laser_hip.h ("F+tree weighted sampler") states it: the tree image
of a row, the guarded draw, update, and draw-and-remove.  float32 throughout, every operation rounded to float32 on its own.
Nothing is read from the code under test.

    image of n weights: P = next power of two >= n, 2 P slots; slot 0 = +0, slot P + i = w[i] (+0 past n),
                        slot j = slot[2 j] + slot[2 j + 1]
    draw(u01):          -1 unless the root is finite and > 0; u = u01 * root; from j = 1 down to a leaf: right when
                        u >= left and right > 0 (u -= left), else left; the result is j - P
"""
import numpy as np

f32 = np.float32


def leaves(n):
    n = int(n)
    assert 1 <= n <= 1 << 24
    p = 1
    while p < n:
        p *= 2
    return p


def tree_elems(n):
    return 2 * leaves(n)


def build(w):
    """tree images of the rows of `w` (1-D: one row): an array (rows, 2 P), level after level from adjacent pairs"""
    w = np.asarray(w, f32)
    w = w.reshape(1, -1) if w.ndim == 1 else w
    rows, n = w.shape
    P = leaves(n)
    t = np.zeros((rows, 2 * P), f32)
    t[:, P:P + n] = w
    with np.errstate(all="ignore"):
        size = P // 2
        while size >= 1:
            t[:, size:2 * size] = (t[:, 2 * size:4 * size:2] + t[:, 2 * size + 1:4 * size:2]).astype(f32)
            size //= 2
    return t


def draw(tree, u01, guard=True):
    """tree: (rows, >= 2 P) images (read only); u01: (rows, m) float32.  Returns int32 (rows, m).  guard=False is the
    reference's rule (no `right > 0` test), kept to show where the two differ."""
    tree = np.asarray(tree, f32)
    u01 = np.asarray(u01, f32)
    rows, m = u01.shape
    P = tree.shape[1] // 2
    assert P & (P - 1) == 0, "the images must be passed without a padded stride"
    rr = np.arange(rows)[:, None]
    with np.errstate(all="ignore"):
        root = tree[:, 1:2]
        ok = np.isfinite(root) & (root > 0)
        u = (u01 * root).astype(f32)
        j = np.ones((rows, m), np.int64)
        while j.flat[0] < P:                      # every descent has the same length
            l, r = tree[rr, 2 * j], tree[rr, 2 * j + 1]
            right = (u >= l) & (r > 0) if guard else (u >= l)
            u = np.where(right, (u - l).astype(f32), u)
            j = 2 * j + right
    return np.where(ok, j - P, -1).astype(np.int32)


def update(tree, elem, weight, n=None):
    """in place: per row, slot[P + elem] = weight and every node above it from its two children; elem == -1 (and, with n
    given, any elem outside [0, n)) is skipped"""
    rows = tree.shape[0]
    P = tree.shape[1] // 2
    elem = np.asarray(elem).reshape(rows)
    weight = np.asarray(weight, f32).reshape(rows)
    with np.errstate(all="ignore"):
        for r in range(rows):
            e = int(elem[r])
            if e < 0 or e >= (P if n is None else n):
                continue
            t = tree[r]
            t[P + e] = weight[r]
            j = (P + e) // 2
            while j >= 1:
                t[j] = f32(t[2 * j] + t[2 * j + 1])
                j //= 2
    return tree


def draw_remove(tree, u01):
    """in place: k = u01.shape[1] draws per row without replacement.  Returns int32 (rows, k); the trees are mutated."""
    u01 = np.asarray(u01, f32)
    rows, k = u01.shape
    out = np.empty((rows, k), np.int32)
    zero = np.zeros(rows, f32)
    for s in range(k):
        idx = draw(tree, u01[:, s:s + 1])[:, 0]
        out[:, s] = idx
        update(tree, idx, zero)
    return out
