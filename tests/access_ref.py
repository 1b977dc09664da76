"""Dry-route reachability, the definition in numpy and plain Python, twice: a heap Dijkstra over (cost, origin) keys and
a literal repeated-sweep relaxation written straight from the move rules of include/floodseg_test.h (mask_access).  Also region_access'
tabulation, access_route, the case generator the CPU and GPU tests share, and the synthetic river scene of the mosaic layer's test."""
import functools
import heapq

import numpy as np

NONE = 0xFFFFFFFF
MAX_COST = 2 ** 31 - 4096
TILE = 32                                                    # FS_ACCESS_TILE: the shapes below are chosen around it
MOVES = ((-1, 0, 5), (1, 0, 5), (0, -1, 5), (0, 1, 5), (-1, -1, 7), (1, -1, 7), (-1, 1, 7), (1, 1, 7))   # (dx, dy, step): W E N S NW NE SW SE
NO_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)


def cost_table(cost):
    table = [0] * 32
    for k, c in (cost.items() if hasattr(cost, "items") else enumerate(cost)):
        table[int(k)] = int(c)
    return table


def class_set(ids):
    bits = 0
    for c in ids:
        bits |= 1 << int(c)
    return bits


def pixel_kinds(mask, cost, terminal):
    """-> (cost per pixel int64 [H,W], 0 on a barrier; passable bool; enterable bool)."""
    table = np.array(cost_table(cost) + [0] * 224, np.int64)
    c = table[mask]
    term = np.zeros(256, bool)
    for k in terminal:
        term[int(k)] = True
    enterable = c > 0
    return c, enterable & ~term[mask], enterable


def move_allowed(k, x, y, passable, enterable):
    """May move k leave pixel (x, y)?  -> the target (qx, qy) or None."""
    h, w = passable.shape
    dx, dy, _ = MOVES[k]
    qx, qy = x + dx, y + dy
    if not (0 <= qx < w and 0 <= qy < h) or not passable[y, x] or not enterable[qy, qx]:
        return None
    if k >= 4 and not (passable[y, qx] and passable[qy, x]):  # the two pixels orthogonally between them: no corner cutting
        return None
    return qx, qy


def dijkstra(mask, seeds, cost, terminal=(), connectivity=8, max_cost=0):
    """One frame.  -> (d uint32 [H,W], origin int32 [H,W]): the minimum over all routes of the pair (total cost, the seed's raster index)."""
    h, w = mask.shape
    c, passable, enterable = pixel_kinds(mask, cost, terminal)
    best = {}
    heap = []
    for y, x in np.argwhere((seeds != 0) & passable).tolist():
        best[(x, y)] = (0, y * w + x)
        heap.append((0, y * w + x, x, y))
    heapq.heapify(heap)
    moves = 8 if connectivity == 8 else 4
    while heap:
        dist, org, x, y = heapq.heappop(heap)
        if best[(x, y)] != (dist, org):
            continue
        for k in range(moves):
            q = move_allowed(k, x, y, passable, enterable)
            if q is None:
                continue
            key = (dist + MOVES[k][2] * int(c[y, x] + c[q[1], q[0]]), org)
            if q not in best or key < best[q]:
                best[q] = key
                heapq.heappush(heap, key + q)
    bound = max_cost or MAX_COST
    d, origin = np.full((h, w), NONE, np.uint32), np.full((h, w), -1, np.int32)
    for (x, y), (dist, org) in best.items():
        if dist <= bound:
            d[y, x], origin[y, x] = dist, org
    return d, origin


def relax(mask, seeds, cost, terminal=(), connectivity=8, max_cost=0, sweeps=None, start=None):
    """The same by repeated sweeps over the whole frame, every pixel gathering from its neighbours, until nothing changes (or `sweeps`
    sweeps).  start = (d, origin): go on from these planes.  -> (d, origin, converged)."""
    h, w = mask.shape
    c, passable, enterable = pixel_kinds(mask, cost, terminal)
    bound = np.uint64(max_cost or MAX_COST)
    if start is None:
        raster = np.arange(h * w, dtype=np.uint64).reshape(h, w)
        key = np.where((seeds != 0) & passable, raster, NO_KEY)
    else:
        key = np.where(start[0] == NONE, NO_KEY, (start[0].astype(np.uint64) << np.uint64(32)) | start[1].astype(np.uint32).astype(np.uint64))

    def shifted(a, dx, dy, fill):  # out[y, x] = a[y + dy, x + dx]
        out = np.full_like(a, fill)
        out[max(-dy, 0):h - max(dy, 0), max(-dx, 0):w - max(dx, 0)] = a[max(dy, 0):h - max(-dy, 0), max(dx, 0):w - max(-dx, 0)]
        return out

    offers = []
    for dx, dy, step in MOVES[:8 if connectivity == 8 else 4]:  # the move from p + (dx, dy) to p
        ok = shifted(passable, dx, dy, False) & enterable
        if dx and dy:
            ok &= shifted(passable, dx, 0, False) & shifted(passable, 0, dy, False)
        offers.append((dx, dy, ok, (step * (shifted(c, dx, dy, 0) + c)).astype(np.uint64)))
    done, converged = 0, False
    while sweeps is None or done < sweeps:
        new = key.copy()
        for dx, dy, ok, wgt in offers:
            nb = shifted(key, dx, dy, NO_KEY)
            total = (nb >> np.uint64(32)) + wgt
            cand = np.where(ok & (nb != NO_KEY) & (total <= bound), nb + (wgt << np.uint64(32)), NO_KEY)
            new = np.minimum(new, cand)
        done += 1
        if np.array_equal(new, key):
            converged = True
            break
        key = new
    d = (key >> np.uint64(32)).astype(np.uint32)
    origin = np.where(key == NO_KEY, -1, (key & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    return d, origin, converged


def mask_access(mask, seeds, cost, terminal=(), connectivity=8, max_cost=0):
    """[n,H,W] -> (d uint32, origin int32, status int32 [n,3]: converged, pixels with a value, 0 -- the status row without its second word,
    which depends on the kernel's tiles)."""
    out = [dijkstra(m, s, cost, terminal, connectivity, max_cost) for m, s in zip(mask, seeds)]
    d, origin = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    status = np.array([[1, int((x != NONE).sum()), 0] for x in d], np.int32)
    return d, origin, status


def real_routes(mask, d, seeds, cost, terminal=(), connectivity=8):
    """Is every value the cost of a real route?  Every valued pixel is a seed that counts with value 0, or has a neighbour q with a value
    and an allowed move q -> p with d[q] + move <= d[p]."""
    h, w = mask.shape
    c, passable, enterable = pixel_kinds(mask, cost, terminal)
    for y, x in np.argwhere(d != NONE).tolist():
        if seeds[y, x] and passable[y, x] and d[y, x] == 0:
            continue
        ok = False
        for k in range(8 if connectivity == 8 else 4):
            dx, dy, step = MOVES[k]
            qx, qy = x + dx, y + dy                                                           # the pixel the move comes from
            if not (0 <= qx < w and 0 <= qy < h) or d[qy, qx] == NONE:
                continue
            back = [j for j in range(8) if MOVES[j][0] == -dx and MOVES[j][1] == -dy][0]
            if move_allowed(back, qx, qy, passable, enterable) == (x, y) and int(d[qy, qx]) + step * int(c[y, x] + c[qy, qx]) <= int(d[y, x]):
                ok = True
                break
        if not ok:
            return False, (x, y)
    return True, None


def access_route(d, mask, cost, terminal, connectivity, x, y):
    """The steepest-descent backtrack from (x, y) to a seed: at every pixel the first neighbour q, in the move table's order, with an
    allowed move q -> p and d[q] + move == d[p].  -> [(x, y), ..., (seed_x, seed_y)]."""
    c, passable, enterable = pixel_kinds(mask, cost, terminal)
    h, w = mask.shape
    if d[y, x] == NONE:
        raise ValueError(f"access_route: ({x}, {y}) has no value")
    chain = [(x, y)]
    while d[y, x] != 0:
        for k in range(8 if connectivity == 8 else 4):
            dx, dy, step = MOVES[k]
            qx, qy = x + dx, y + dy
            if not (0 <= qx < w and 0 <= qy < h) or d[qy, qx] == NONE:
                continue
            back = [j for j in range(8) if MOVES[j][0] == -dx and MOVES[j][1] == -dy][0]
            if move_allowed(back, qx, qy, passable, enterable) == (x, y) and int(d[qy, qx]) + step * int(c[y, x] + c[qy, qx]) == int(d[y, x]):
                x, y = qx, qy
                break
        else:
            raise ValueError(f"access_route: no neighbour of ({x}, {y}) explains its value: the field is not converged")
        chain.append((x, y))
    return chain


def route_cost(chain, mask, cost):
    table = cost_table(cost)
    total = 0
    for (x0, y0), (x1, y1) in zip(chain, chain[1:]):
        assert max(abs(x0 - x1), abs(y0 - y1)) == 1
        total += (7 if x0 != x1 and y0 != y1 else 5) * (table[mask[y0, x0]] + table[mask[y1, x1]])
    return total


# ------------------------------------------------------------------------------------------------ the tabulation
def region_access(mask, d, origin, index, counts, classes, max_regions):
    """[n,H,W] planes, region_table's index and counts -> (reach int64 [n,K,4], rows int64 [n,max_regions,8])."""
    n, h, w = mask.shape
    reach, rows = np.zeros((n, classes, 4), np.int64), np.zeros((n, max_regions, 8), np.int64)
    for f in range(n):
        has = d[f] != NONE
        for k in range(classes):
            of = mask[f] == k
            v = d[f][of & has].astype(np.int64)
            reach[f, k] = (of.sum(), v.size, v.sum(), v.max() if v.size else 0)
        written = min(max(int(counts[f, 1]), 0), max_regions)
        for r in range(written):
            at = np.flatnonzero((index[f].reshape(-1) == r) & has.reshape(-1))
            if not at.size:
                rows[f, r] = (-1, -1, -1, -1, -1, -1, 0, -1)
                continue
            v = d[f].reshape(-1)[at].astype(np.int64)
            p = int(at[np.argmin(v)])                                  # argmin: the first of several, the lowest raster index
            row = [int(v.min()), p % w, p // w, -1, -1, -1, int(at.size), int(v.max())]
            if origin is not None:
                q = int(origin[f].reshape(-1)[p])
                i = int(index[f].reshape(-1)[q])
                row[3:6] = q % w, q // w, i if 0 <= i < written else -1
            rows[f, r] = row
    return reach, rows


# ------------------------------------------------------------------------------------------------ the cases
def random_case(seed, h, w, n=1, blocks=True):
    """Five-class masks with blobs and speckle, a few ids >= 32 and 255 among them; costs that include 1 and 255, water (1) a barrier,
    buildings (3) terminal; seeds partly on barriers and terminals."""
    rng = np.random.default_rng(seed)
    if blocks:
        coarse = rng.choice(5, size=(n, -(-h // 3), -(-w // 3)), p=[0.4, 0.15, 0.15, 0.1, 0.2])
        mask = np.repeat(np.repeat(coarse, 3, 1), 3, 2)[:, :h, :w]
    else:
        mask = rng.choice(5, size=(n, h, w), p=[0.4, 0.15, 0.15, 0.1, 0.2])
    speck = rng.random((n, h, w))
    mask = np.where(speck < 0.08, rng.integers(0, 5, (n, h, w)), mask)
    mask = np.where(speck > 0.99, rng.choice([32, 200, 255], size=(n, h, w)), mask).astype(np.uint8)
    cost = [int(v) for v in rng.integers(1, 256, 5)]
    cost[1], cost[int(rng.integers(2, 4))], cost[4 if seed % 2 else 0] = 0, 255, 1
    seeds = (rng.random((n, h, w)) < max(0.002, 3.0 / (h * w))).astype(np.uint8) * rng.integers(1, 256, (n, h, w)).astype(np.uint8)
    return mask, seeds, cost, (3,)


def serpentine(h=96, w=130):
    """A corridor of streets one pixel wide that runs every even row from end to end and turns through a one-pixel gap in the wall of
    water below it, at alternating ends: about h * w / 2 pixels long, across every tile border of the frame dozens of times."""
    mask = np.full((1, h, w), 4, np.uint8)
    mask[0, 1::2] = 1
    for i, y in enumerate(range(1, h, 2)):
        mask[0, y, w - 1 if i % 2 == 0 else 0] = 4
    seeds = np.zeros((1, h, w), np.uint8)
    seeds[0, 0, 0] = 1
    return mask, seeds, [2, 0, 6, 9, 1], (3,)


def junction():
    """Two seeds at equal cost from a junction: a street from (2, 20) to (62, 20), seeds at both ends, a side street down from its middle
    (32, 20) to a building.  Everything on the side street is as far from either seed: the origin is the one with the lower index."""
    mask = np.full((1, 45, 65), 1, np.uint8)
    mask[0, 20, 2:63] = 4
    mask[0, 21:40, 32] = 4
    mask[0, 40, 32] = 3
    seeds = np.zeros((1, 45, 65), np.uint8)
    seeds[0, 20, 2] = seeds[0, 20, 62] = 7
    return mask, seeds, [2, 0, 6, 9, 1], (3,)


def op_cases():
    """(name, mask, seeds, cost, terminal, connectivity) -- every content and shape the issue lists, at the smallest sizes that hold it."""
    cases = []
    for i, (h, w) in enumerate([(1, 1), (1, 37), (41, 1)] + [(a, b) for a in (TILE - 1, TILE, TILE + 1) for b in (TILE - 1, TILE, TILE + 1)]):
        m, s, c, t = random_case(100 + i, h, w, blocks=h > 1 and w > 1)
        if h * w == 1:
            m[:], s[:] = 4, 1
        if h == 1 or w == 1:
            m[m == 1] = 0                                          # a line with a barrier every few pixels reaches nothing
        walk = np.argwhere((m[0] < 5) & (m[0] != 1) & (m[0] != 3))
        s[0, walk[len(walk) // 3][0], walk[len(walk) // 3][1]] = 9  # at least one seed that counts
        cases.append((f"{h}x{w}", m, s, c, t, 8 if i % 3 else 4))
    m, s, c, t = random_case(7, 70, 150, n=3)
    s[1] = np.where((m[1] == 1) | (m[1] == 3) | (m[1] >= 32), s[1], 0)            # frame 1: seeds on barriers and terminals only: no valid seed
    s[1, 0, 0], m[1, 0, 0] = 1, 1
    m[2], s[2] = 0, 0                                                                # frame 2: all passable, one seed
    s[2, 50, 11] = 1
    cases.append(("70x150x3", m, s, c, t, 8))
    cases.append(("70x150x3 conn4", m, s, c, t, 4))
    m, s, c, t = random_case(9, 66, 97, blocks=False)
    cases.append(("speckle 66x97", m, s, c, t, 8))
    cases.append(("junction",) + junction() + (8,))
    return cases


@functools.lru_cache(maxsize=None)
def case_reference(name, max_cost=0):
    case = [c for c in op_cases() if c[0] == name][0]
    return mask_access(case[1], case[2], case[3], case[4], case[5], max_cost)


@functools.lru_cache(maxsize=None)
def serpentine_reference():
    m, s, c, t = serpentine()
    return mask_access(m, s, c, t, 8, 0)


# ------------------------------------------------------------------------------------------------ the mosaic layer's scene
SCENE = (120, 160)
SCENE_COST = {4: 1, 0: 2, 2: 6, 3: 2}                        # the defaults of flow.mosaic.mosaic_access: street, background, tree, building
BRIDGE_ROWS, RIVER = (58, 61), (70, 90)                      # the bridge: three rows of street across the river's columns
NEAR_BUILDINGS = [(10, 10, 18, 22), (80, 20, 90, 34), (100, 8, 108, 16)]       # (y0, x0, y1, x1), left bank
FAR_BUILDINGS = [(12, 122, 20, 136), (70, 120, 82, 130), (98, 100, 106, 112), (40, 140, 46, 150)]
SCENE_SEED = (5, 60)                                         # (x, y): on the left bank's street


def scene_classes(cut=False):
    """Two banks of background with trees, a river, one bridge, streets and buildings on both sides; a margin never seen (255)."""
    h, w = SCENE
    cls = np.zeros((h, w), np.uint8)
    cls[:, RIVER[0]:RIVER[1]] = 1
    cls[BRIDGE_ROWS[0]:BRIDGE_ROWS[1], 4:w - 4] = 4              # the road over the bridge
    cls[30:36, 20:50] = 2
    cls[64:90, 100:104] = 2
    cls[8:112, 40:42] = 4
    cls[8:112, 116:118] = 4
    for y0, x0, y1, x1 in NEAR_BUILDINGS + FAR_BUILDINGS:
        cls[y0:y1, x0:x1] = 3
    cls[:3], cls[-3:], cls[:, :2], cls[:, -2:] = 255, 255, 255, 255
    if cut:
        cls[BRIDGE_ROWS[0]:BRIDGE_ROWS[1], 80] = 1               # three bridge pixels voted to water
    return cls


def scene_votes(cut=False, classes=5):
    """The scene as a vote canvas uint16 [K, CH, CW]: the class gets 5 votes, another one 2; unseen ground none."""
    cls = scene_classes(cut)
    votes = np.zeros((classes,) + SCENE, np.uint16)
    for k in range(classes):
        votes[k][cls == k] = 5
        votes[(k + 1) % classes][cls == k] += 2
    return votes


def access_csv_lines(table, written, rows, converged, class_names=None):
    """flow.mosaic.write_access_csv's lines from region_table's rows and region_access' rows of one frame."""
    name = (lambda c: str(c)) if class_names is None else (lambda c: str(class_names[c]))
    lines = ["region,class,area,centroid_x,centroid_y,state,cost,at_x,at_y,origin_x,origin_y,origin_region"]
    for r in range(written):
        t, a = [int(v) for v in table[r]], [int(v) for v in rows[r]]
        state = ("reached" if converged else "reached_bound") if a[0] >= 0 else ("cut_off" if converged else "not_reached_yet")
        vals = [str(v) if a[0] >= 0 else "" for v in a[:5]] + [str(a[5]) if a[0] >= 0 and a[5] >= 0 else ""]
        lines.append(",".join([str(r), name(t[0]), str(t[1]), f"{t[6] / t[1]:.2f}", f"{t[7] / t[1]:.2f}", state] + vals))
    return lines + [""]
