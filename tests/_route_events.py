"""Random route table pairs and the numpy restatement of the action rule (include/holo_spf_hip.h, HSPF_DIFF_*) for the
tests of hspf_routes_events.  Nothing here touches the GPU."""
import numpy as np

SAME, INSTALL, WITHDRAW, SILENT = 0, 1, 2, 3
NONE = 0xFFFFFFFF
REC = 8


def _draw(rng, shape, W, p_none=0.15, p_no_nh=0.2):
    """Tables as hspf_routes_device writes them: no route = (INF, NONE, 0); a route has a metric, an entry and a mask that
    may be empty (CONNECTED / unresolved)."""
    n = int(np.prod(shape))
    none = rng.random(n) < p_none
    bm = rng.integers(1, 1000, n, dtype=np.uint32)
    be = rng.integers(0, 1 << 20, n, dtype=np.uint32)
    nm = rng.integers(1, 1 << 63, (n, W), dtype=np.uint64) * (rng.random((n, W)) < 0.7)
    nm[:, 0] |= np.uint64(1) << rng.integers(0, 64, n, dtype=np.uint64)         # at least one next hop ...
    nm[rng.random(n) < p_no_nh] = 0                                             # ... unless the route has none
    bm[none], be[none], nm[none] = NONE, NONE, 0
    return bm.reshape(shape), be.reshape(shape), nm.reshape(shape + (W,))


def table_pair(seed, R, P, W, density):
    """(old, new): `density` of the pairs re-drawn (1.0: every pair is an event, 0.0: identical tables)."""
    rng = np.random.default_rng(seed)
    if density >= 1.0:
        old = _draw(rng, (R, P), W, p_none=0.0)
        new = _draw(rng, (R, P), W)
        has = new[1] != NONE
        new[0][has] = old[0][has] + 1000                     # a route that stays changes its metric: never SAME
        return old, new
    old = _draw(rng, (R, P), W)
    new = tuple(a.copy() for a in old)
    if density > 0.0:
        n = R * P
        k = max(1, int(round(n * density)))
        idx = rng.choice(n, size=k, replace=False)
        fresh = _draw(rng, (k,), W, p_none=0.3, p_no_nh=0.3)
        for dst, src in zip(new, fresh):
            dst.reshape((n,) + dst.shape[2:])[idx] = src
        same = actions(old, new) == SAME                     # the rule compares metric and next hops: an entry alone does not change
        new[1][same] = old[1][same]
    return old, new


def actions(old, new):
    (om, oe, on), (nm, ne, nn) = old, new
    had, has = oe != NONE, ne != NONE
    same_nh = (on == nn).all(-1)
    old_nh, new_nh = (on != 0).any(-1), (nn != 0).any(-1)
    return np.where(has, np.where(had & (om == nm) & same_nh, SAME, np.where(new_nh, INSTALL, SILENT)),
                    np.where(had, np.where(old_nh, WITHDRAW, SILENT), SAME)).astype(np.uint32)


def want_stream(old, new, with_silent):
    """The stream the header describes, built in numpy: [n, 8 + 4 W] u32 in pair order."""
    (om, oe, on), (nm, ne, nn) = old, new
    R, P, W = on.shape
    act = actions(old, new)
    sel = (act == INSTALL) | (act == WITHDRAW) | ((act == SILENT) if with_silent else False)
    r, p = np.nonzero(sel)                                   # row-major: roots ascending, prefixes ascending inside a root
    rec = np.zeros((len(r), REC + 4 * W), np.uint32)
    rec[:, 0], rec[:, 1], rec[:, 2] = r, p, act[r, p]
    rec[:, 3], rec[:, 4], rec[:, 5], rec[:, 6] = nm[r, p], ne[r, p], om[r, p], oe[r, p]
    rec[:, REC:REC + 2 * W] = np.ascontiguousarray(nn[r, p]).view(np.uint32).reshape(len(r), 2 * W)
    rec[:, REC + 2 * W:] = np.ascontiguousarray(on[r, p]).view(np.uint32).reshape(len(r), 2 * W)
    return rec
