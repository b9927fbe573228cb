"""Numpy restatement of the section "rasterising an indexed mesh" of include/vacancy_hip.h, step by step, and its named
mutants.  Float steps are numpy float32 scalars (each operation rounded on its own), the per-pixel steps numpy float64.

`rules`: a set of mutant names, each turning ONE rule of the definition (tests/test_raster_cpu.py shows that the cases
tell every one of them from the definition):
  "open"     coverage s * e_k > 0 instead of >= 0
  "nocanon"  the edge function not canonicalised: evaluated from the face's own first vertex of the edge
  "tiehigh"  of two fragments with equal depth bits the HIGHER face index wins
  "boxswap"  the box from floorf(min) to ceilf(max)
  "affine"   the ortho depth formula in a pinhole view
  "zlt"      a pinhole vertex is unusable for pc[2] < 0 instead of <= 0
"""
import numpy as np

F = np.float32
D = np.float64
MUTANTS = ("open", "nocanon", "tiehigh", "boxswap", "affine", "zlt")


def project(view, p, rules=frozenset()):
    """Step 1: (u, w, z, usable) of the float32 point p."""
    with np.errstate(all="ignore"):
        R = [[F(view.w2c[4 * r + c]) for c in range(3)] for r in range(3)]
        t = [F(view.w2c[4 * r + 3]) for r in range(3)]
        px, py, pz = F(p[0]), F(p[1]), F(p[2])
        pc = [t[r] + (R[r][0] * px + (R[r][1] * py + R[r][2] * pz)) for r in range(3)]
        if view.is_ortho:
            u, w = pc[0], pc[1]
            front = not (pc[2] < 0)
        else:
            u = F(view.fx) / pc[2] * pc[0] + F(view.cx)
            w = F(view.fy) / pc[2] * pc[1] + F(view.cy)
            front = bool(pc[2] >= 0) if "zlt" in rules else bool(pc[2] > 0)
        usable = front and all(np.isfinite(x) for x in (pc[0], pc[1], pc[2], u, w))
    return u, w, pc[2], bool(usable)


def edge_value(i, j, a, b, px, py, rules=frozenset()):
    """Step 3: the face's value at (px, py) for its directed edge from vertex i (at a = (u, w)) to vertex j (at b)."""
    forward = i < j or "nocanon" in rules
    if not forward:
        a, b = b, a
    ax, ay, bx, by = D(a[0]), D(a[1]), D(b[0]), D(b[1])
    e = (bx - ax) * (D(py) - ay) - (by - ay) * (D(px) - ax)
    return e if forward else -e


def raster_view(vertices, faces, view, rules=frozenset(), stats=None):
    """One view: (depth float32 [h, w], face int32 [h, w], hits uint64 [h, (w + 63) // 64], n_dropped int64 [2]).
    `stats`: a dict that receives "boxes" (candidate pixels of every drawn face, in face order) and "ties" (how often two
    fragments with equal depth bits met in a pixel) -- what the tests show their cases to reach."""
    rules = frozenset(rules)
    w, h = view.width, view.height
    best = {}  # (x, y) -> (depth bits, face)
    dropped = np.zeros(2, np.int64)
    boxes, ties = [], 0
    proj = [project(view, v, rules) for v in np.asarray(vertices, np.float32).reshape(-1, 3)]
    with np.errstate(all="ignore"):
        for fi, ids in enumerate(np.asarray(faces, np.int32).reshape(-1, 3)):
            ids = [int(k) for k in ids]
            P = [proj[k] for k in ids]
            if not all(p[3] for p in P):
                dropped[0] += 1
                continue
            if len(set(ids)) < 3:
                dropped[1] += 1
                continue
            uw = [(p[0], p[1]) for p in P]
            A = edge_value(ids[0], ids[1], uw[0], uw[1], uw[2][0], uw[2][1], rules)
            if not (A > 0 or A < 0) or not np.isfinite(A):
                dropped[1] += 1
                continue
            s = D(1.0) if A > 0 else D(-1.0)
            us, ws = [p[0] for p in P], [p[1] for p in P]
            lo, hi = (np.floor, np.ceil) if "boxswap" in rules else (np.ceil, np.floor)
            x0 = max(lo(min(us)), F(view.roi_min[0]))
            x1 = min(hi(max(us)), F(view.roi_max[0]))
            y0 = max(lo(min(ws)), F(view.roi_min[1]))
            y1 = min(hi(max(ws)), F(view.roi_max[1]))
            if not (x0 <= x1 and y0 <= y1):
                boxes.append(0)
                continue
            boxes.append((int(x1) - int(x0) + 1) * (int(y1) - int(y0) + 1))
            z = [D(p[2]) for p in P]
            for y in range(int(y0), int(y1) + 1):
                for x in range(int(x0), int(x1) + 1):
                    e = [edge_value(ids[1], ids[2], uw[1], uw[2], x, y, rules),
                         edge_value(ids[2], ids[0], uw[2], uw[0], x, y, rules),
                         edge_value(ids[0], ids[1], uw[0], uw[1], x, y, rules)]
                    if "open" in rules:
                        covered = all(s * ek > 0 for ek in e)
                    else:
                        covered = all(s * ek >= 0 for ek in e)
                    if not covered:
                        continue
                    l = [ek / A for ek in e]
                    if view.is_ortho or "affine" in rules:
                        zz = (l[0] * z[0] + l[1] * z[1]) + l[2] * z[2]
                    else:
                        zz = D(1.0) / ((l[0] * (D(1.0) / z[0]) + l[1] * (D(1.0) / z[1])) + l[2] * (D(1.0) / z[2]))
                    d = F(zz)
                    if not np.isfinite(d) or d < 0:
                        continue
                    if d == 0:
                        d = F(0.0)
                    key = (int(np.array(d, np.float32).view(np.uint32)), fi)
                    old = best.get((x, y))
                    ties += old is not None and old[0] == key[0]
                    if old is None:
                        better = True
                    elif "tiehigh" in rules:
                        better = key[0] < old[0] or (key[0] == old[0] and key[1] > old[1])
                    else:
                        better = key < old
                    if better:
                        best[(x, y)] = key
    if stats is not None:
        stats["boxes"], stats["ties"] = boxes, int(ties)
    depth = np.full((h, w), np.inf, np.float32)
    face = np.full((h, w), -1, np.int32)
    hits = np.zeros((h, (w + 63) // 64), np.uint64)
    for (x, y), (bits, fi) in best.items():
        depth[y, x] = np.array(bits, np.uint32).view(np.float32)
        face[y, x] = fi
        hits[y, x >> 6] |= np.uint64(1) << np.uint64(x & 63)
    return depth, face, hits, dropped


def raster(vertices, faces, views, rules=frozenset()):
    """All views: a list of dicts shaped like carver.raster_mesh_host's."""
    out = []
    for view in views:
        d, f, hb, nd = raster_view(vertices, faces, view, rules)
        out.append({"depth": d, "face": f, "hits": hb, "n_dropped": nd})
    return out


def same(a, b):
    """Two lists of result dicts agree in depth bits, face ids, hit words and drops."""
    return len(a) == len(b) and all(
        np.array_equal(x["depth"].view(np.uint32), y["depth"].view(np.uint32)) and np.array_equal(x["face"], y["face"])
        and np.array_equal(x["hits"], y["hits"]) and np.array_equal(x["n_dropped"], y["n_dropped"]) for x, y in zip(a, b))
