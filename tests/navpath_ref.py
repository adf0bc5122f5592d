"""The path contract of include/gem_hip_navpath.h in numpy scalar float32 / float64 operations, written twice.

  walk_literal   global_planner's GradientPath::getPath and gradCell as recalled (ROS noetic, unverified against the library): ONE linear
                 index stc into a float potential array, its neighbours at stc +- 1 and stc +- xs, POT_HIGH = 1e10, and the gradx_ /
                 grady_ cache arrays that gradCell fills and consults.  The library has no column check and relies on the outline; so
                 that the linear index never wraps, the literal version runs over the potential framed by two rings of high cells (the
                 points are still formed from the unframed coordinates: a float add rounds by its operands).
  walk           the pure function of the header: P(x, y) with UNREACHED off the map, int32 differences converted to float, the gradient
                 of a cell recomputed whenever it is asked for.

tests/test_navpath_cpu.py asserts that the two agree on every case: the cache is inert, and float differences equal int32 differences
while potentials stay below 2^24.  Every float operation is one numpy scalar operation, so each is rounded on its own.
Potentials are int32 [size_y, size_x]; cells are (x, y); points are (float32, float32) in walk order, goal first."""
import numpy as np

UNREACHED = 0x7FFFFFFF
GRID, GRADIENT = 0, 1
FOUND, OFF_MAP, UNREACHED_GOAL, HIGH, ZERO_GRADIENT, CAP = 1, 2, 3, 4, 5, 6
F32, F64 = np.float32, np.float64
# the fallback's scan: row-major, NOT the grid path's order
FALLBACK = [(-1, -1), (0, -1), (1, -1), (-1, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]
# the grid path's order (navplan_ref.NEIGHBOURS)
GRID_ORDER = [(xd, yd) for xd in (-1, 0, 1) for yd in (-1, 0, 1) if (xd, yd) != (0, 0)]


def result(status, n, goal, gp):
    return {"status": status, "n_points": n, "goal_cell": goal, "goal_potential": gp}


def words(r):
    """the eight int32 words of gem_navpath_result"""
    return [r["status"], r["n_points"], r["goal_cell"][0], r["goal_cell"][1], r["goal_potential"], 0, 0, 0]


def _lerp(t, a, b):
    """(float)((1.0 - (double)t) * (double)a + (double)(t * b))"""
    return F32((F64(1.0) - F64(t)) * F64(a) + F64(F32(t * b)))


# ---- the pure function -----------------------------------------------------------------------------------------------------------------
def walk(pot, start, goal, max_points, info=None):
    """the GRADIENT walk; returns (points, result).  info (a dict) counts the fallbacks taken: 'high', 'osc' (osc alone)"""
    sy, sx = pot.shape
    sx0, sy0 = int(start[0]), int(start[1])
    gx, gy = int(goal[0]), int(goal[1])

    def P(x, y):
        return int(pot[y, x]) if 0 <= x < sx and 0 <= y < sy else UNREACHED

    def G(x, y):
        cv = P(x, y)
        gx_, gy_ = F32(0), F32(0)
        if P(x - 1, y) != UNREACHED: gx_ = gx_ + F32(P(x - 1, y) - cv)
        if P(x + 1, y) != UNREACHED: gx_ = gx_ + F32(cv - P(x + 1, y))
        if P(x, y - 1) != UNREACHED: gy_ = gy_ + F32(P(x, y - 1) - cv)
        if P(x, y + 1) != UNREACHED: gy_ = gy_ + F32(cv - P(x, y + 1))
        n = np.sqrt(F32(F32(gx_ * gx_) + F32(gy_ * gy_)))
        if n > 0:
            r = F32(F64(1.0) / F64(n))
            return F32(r * gx_), F32(r * gy_)
        return F32(0), F32(0)

    if not (0 <= gx < sx and 0 <= gy < sy):
        return [], result(OFF_MAP, 0, (-1, -1), UNREACHED)
    if P(gx, gy) == UNREACHED:
        return [], result(UNREACHED_GOAL, 0, (gx, gy), UNREACHED)
    gp = P(gx, gy)
    cx, cy, dx, dy = gx, gy, F32(0), F32(0)
    pts = []
    while True:
        if len(pts) >= max_points:
            return pts, result(CAP, len(pts), (gx, gy), gp)
        nx, ny = F32(F32(cx) + dx), F32(F32(cy) + dy)
        if abs(F64(nx) - F64(sx0)) < 0.5 and abs(F64(ny) - F64(sy0)) < 0.5:
            pts.append((F32(sx0), F32(sy0)))
            return pts, result(FOUND, len(pts), (gx, gy), gp)
        pts.append((nx, ny))
        osc = len(pts) > 2 and pts[-1][0] == pts[-3][0] and pts[-1][1] == pts[-3][1]
        high = any(P(cx + i, cy + j) == UNREACHED for j in (-1, 0, 1) for i in (-1, 0, 1))
        if high or osc:
            if info is not None:
                info["high" if high else "osc"] = info.get("high" if high else "osc", 0) + 1
            best, bp = (cx, cy), P(cx, cy)
            for i, j in FALLBACK:
                if P(cx + i, cy + j) < bp:
                    best, bp = (cx + i, cy + j), P(cx + i, cy + j)
            cx, cy = best
            dx, dy = F32(0), F32(0)
            if P(cx, cy) == UNREACHED:
                return pts, result(HIGH, len(pts), (gx, gy), gp)
            continue
        g00, g10, g01, g11 = G(cx, cy), G(cx + 1, cy), G(cx, cy + 1), G(cx + 1, cy + 1)
        x = _lerp(dy, _lerp(dx, g00[0], g10[0]), _lerp(dx, g01[0], g11[0]))
        y = _lerp(dy, _lerp(dx, g00[1], g10[1]), _lerp(dx, g01[1], g11[1]))
        if x == 0 and y == 0:
            return pts, result(ZERO_GRADIENT, len(pts), (gx, gy), gp)
        ss = F32(F32(0.5) / np.sqrt(F32(F32(x * x) + F32(y * y))))
        dx = F32(dx + F32(x * ss))
        dy = F32(dy + F32(y * ss))
        if dx > 1: cx += 1; dx = F32(dx - F32(1))
        if dx < -1: cx -= 1; dx = F32(dx + F32(1))
        if dy > 1: cy += 1; dy = F32(dy - F32(1))
        if dy < -1: cy -= 1; dy = F32(dy + F32(1))


# ---- the literal version -----------------------------------------------------------------------------------------------------------------
POT_HIGH = F32(1.0e10)
PAD = 2


def walk_literal(pot, start, goal, max_points):
    """GradientPath::getPath with its linear index and its gradient cache, over the framed float potential; (points, result)"""
    sy, sx = pot.shape
    sx0, sy0 = int(start[0]), int(start[1])
    gx, gy = int(goal[0]), int(goal[1])
    if not (0 <= gx < sx and 0 <= gy < sy):
        return [], result(OFF_MAP, 0, (-1, -1), UNREACHED)
    if int(pot[gy, gx]) == UNREACHED:
        return [], result(UNREACHED_GOAL, 0, (gx, gy), UNREACHED)
    reached = pot != UNREACHED
    assert not reached.any() or int(pot[reached].max()) < (1 << 24), "float potentials are exact below 2^24 only"
    xs, ys = sx + 2 * PAD, sy + 2 * PAD
    framed = np.full((ys, xs), POT_HIGH, F32)
    framed[PAD:PAD + sy, PAD:PAD + sx] = np.where(reached, pot, 0).astype(F32)
    framed[PAD:PAD + sy, PAD:PAD + sx][~reached] = POT_HIGH
    potential = framed.reshape(-1)
    gradx, grady = np.zeros(xs * ys, F32), np.zeros(xs * ys, F32)

    def grad_cell(n):
        if F32(gradx[n] + grady[n]) > 0.0:                               # the cache's test, as the library has it
            return
        if n < xs or n > xs * ys - xs:
            return
        cv = potential[n]
        dx, dy = F32(0), F32(0)
        assert cv < POT_HIGH                                             # (the library's branch for a high cell is dead in this walk)
        if potential[n - 1] < POT_HIGH: dx = F32(dx + F32(potential[n - 1] - cv))
        if potential[n + 1] < POT_HIGH: dx = F32(dx + F32(cv - potential[n + 1]))
        if potential[n - xs] < POT_HIGH: dy = F32(dy + F32(potential[n - xs] - cv))
        if potential[n + xs] < POT_HIGH: dy = F32(dy + F32(cv - potential[n + xs]))
        norm = np.sqrt(F32(F32(dx * dx) + F32(dy * dy)))
        if norm > 0:
            norm = F32(F64(1.0) / F64(norm))
            gradx[n] = F32(norm * dx)
            grady[n] = F32(norm * dy)

    stc = (gy + PAD) * xs + gx + PAD
    dx, dy = F32(0), F32(0)
    path = []
    gp = int(pot[gy, gx])
    while True:
        if len(path) >= max_points:                                      # (the library: 4 * xs * ys iterations and an empty plan)
            return path, result(CAP, len(path), (gx, gy), gp)
        nx, ny = F32(F32(stc % xs - PAD) + dx), F32(F32(stc // xs - PAD) + dy)
        if abs(F64(nx) - F64(sx0)) < 0.5 and abs(F64(ny) - F64(sy0)) < 0.5:
            path.append((F32(sx0), F32(sy0)))
            return path, result(FOUND, len(path), (gx, gy), gp)
        assert not (stc < xs or stc > xs * ys - xs)                      # the library's row guard: never met inside the frame
        path.append((nx, ny))
        npath = len(path)
        oscillation_detected = npath > 2 and path[npath - 1][0] == path[npath - 3][0] and path[npath - 1][1] == path[npath - 3][1]
        stcnx, stcpx = stc + xs, stc - xs
        if (potential[stc] >= POT_HIGH or potential[stc + 1] >= POT_HIGH or potential[stc - 1] >= POT_HIGH or potential[stcnx] >= POT_HIGH
                or potential[stcnx + 1] >= POT_HIGH or potential[stcnx - 1] >= POT_HIGH or potential[stcpx] >= POT_HIGH
                or potential[stcpx + 1] >= POT_HIGH or potential[stcpx - 1] >= POT_HIGH or oscillation_detected):
            minc, minp = stc, potential[stc]
            for st in (stcpx - 1, stcpx, stcpx + 1, stc - 1, stc + 1, stcnx - 1, stcnx, stcnx + 1):
                if potential[st] < minp:
                    minp, minc = potential[st], st
            stc = minc
            dx, dy = F32(0), F32(0)
            if potential[stc] >= POT_HIGH:
                return path, result(HIGH, len(path), (gx, gy), gp)
        else:
            grad_cell(stc); grad_cell(stc + 1); grad_cell(stcnx); grad_cell(stcnx + 1)
            x1 = _lerp(dx, gradx[stc], gradx[stc + 1])
            x2 = _lerp(dx, gradx[stcnx], gradx[stcnx + 1])
            x = _lerp(dy, x1, x2)
            y1 = _lerp(dx, grady[stc], grady[stc + 1])
            y2 = _lerp(dx, grady[stcnx], grady[stcnx + 1])
            y = _lerp(dy, y1, y2)
            if x == 0.0 and y == 0.0:
                return path, result(ZERO_GRADIENT, len(path), (gx, gy), gp)
            ss = F32(F32(0.5) / np.sqrt(F32(F32(x * x) + F32(y * y))))
            dx = F32(dx + F32(x * ss))
            dy = F32(dy + F32(y * ss))
            if dx > 1.0: stc += 1; dx = F32(dx - F32(1))
            if dx < -1.0: stc -= 1; dx = F32(dx + F32(1))
            if dy > 1.0: stc += xs; dy = F32(dy - F32(1))
            if dy < -1.0: stc -= xs; dy = F32(dy + F32(1))


# ---- the grid form -------------------------------------------------------------------------------------------------------------------------
def walk_grid(pot, start, goal, max_points):
    """the GRID form: the grid path's walk, cells as float points, goal first; (points, result)"""
    sy, sx = pot.shape
    gx, gy = int(goal[0]), int(goal[1])
    if not (0 <= gx < sx and 0 <= gy < sy):
        return [], result(OFF_MAP, 0, (-1, -1), UNREACHED)
    gp = int(pot[gy, gx])
    if gp == UNREACHED:
        return [], result(UNREACHED_GOAL, 0, (gx, gy), UNREACHED)
    c = (gx, gy)
    pts = []
    while True:
        if len(pts) >= max_points:
            return pts, result(CAP, len(pts), (gx, gy), gp)
        pts.append((F32(c[0]), F32(c[1])))
        if c == (int(start[0]), int(start[1])):
            return pts, result(FOUND, len(pts), (gx, gy), gp)
        best, nxt = None, None
        for xd, yd in GRID_ORDER:
            x, y = c[0] + xd, c[1] + yd
            if 0 <= x < sx and 0 <= y < sy and (best is None or int(pot[y, x]) < best):
                best, nxt = int(pot[y, x]), (x, y)
        if nxt is None:
            return pts, result(HIGH, len(pts), (gx, gy), gp)
        c = nxt


def points_array(pts):
    return np.array([[p[0], p[1]] for p in pts], np.float32).reshape(-1, 2)
