"""The dash specification of include/vgx.h ("dashed strokes") as a plain sequential program: the model vgx_dash is pinned to.

One list at a time, one "on" interval at a time in the order r = 0, 1, ... / k = 0, 2, ..., one cursor that walks the list's
vertices forwards. Python ints for everything in fixed point, numpy float32 scalars for the three float steps (segment length, the
interpolation parameter, the interpolated point), so every operation is rounded exactly once to the format the specification names.
Nothing here is shared with csrc/vgx_dash.h: that code finds intervals by a division and vertices by binary search."""
import numpy as np

f32 = np.float32
SNAP = 256                      # D
MAX_T = 1 << 62                 # longest list
MAX_ENTRY = float(1 << 40)      # entries and phase lie below it
MAX_LEN = float(1 << 46)        # a longer segment alone exceeds MAX_T
MAX_INTERVALS = (1 << 32) - 1
DASH_MAX = 32
OK, E_INVALID_ARG, E_NOSPACE, E_RANGE = 0, 1, 4, 8

subpath_dtype = np.dtype([("first_vertex", "<u8"), ("num_vertices", "<u4"), ("flags", "<u4")])
dash_dtype = np.dtype([("first", "<u4"), ("count", "<u4"), ("phase", "<f4"), ("reserved", "<u4")])


def q(x):
    return int(float(x) * 65536.0 + 0.5)


def entry_ok(x):
    x = float(x)
    return np.isfinite(x) and 0.0 <= x < MAX_ENTRY


def pattern_of(rec, pattern):
    """(A, P, f) of one record, or None when it breaks a rule. count == 0: ([0], 0, 0)."""
    first, count = int(rec["first"]), int(rec["count"])
    if int(rec["reserved"]) != 0 or count % 2 or count > DASH_MAX or first + count > len(pattern) or not entry_ok(rec["phase"]):
        return None
    A = [0]
    for k in range(count):
        if not entry_ok(pattern[first + k]):
            return None
        A.append(A[-1] + q(pattern[first + k]))
    if count == 0:
        return A, 0, 0
    if A[-1] == 0:
        return None
    return A, A[-1], q(rec["phase"]) % A[-1]


def validate(dashes, pattern):
    if not all(entry_ok(p) for p in pattern):
        return E_INVALID_ARG
    return OK if all(pattern_of(r, pattern) is not None for r in dashes) else E_INVALID_ARG


class Range(Exception):
    pass


def prefix_lengths(V, closed):
    """S_0 .. S_m of a list (python ints)."""
    n = len(V)
    m = 0 if n < 2 else (n if closed else n - 1)
    S = [0]
    for i in range(m):
        a, b = V[i], V[(i + 1) % n]
        with np.errstate(all="ignore"):
            dx = f32(b[0] - a[0])
            dy = f32(b[1] - a[1])
            ln = np.sqrt(f32(f32(dx * dx) + f32(dy * dy)))
        if not (ln < MAX_LEN):
            raise Range()
        S.append(S[-1] + q(ln))
    if S[-1] > MAX_T:
        raise Range()
    return S


def interval_count(A, P, f, T):
    """The "on" intervals (r, k) that can meet [0, T]: r P + A_k - f < T and r P + A_{k+1} - f > 0, counted entry by entry."""
    total = 0
    if T == 0:
        return 0
    for k in range(0, len(A) - 1, 2):
        if T + f - A[k] < 1:
            continue
        r_max = (T + f - A[k] - 1) // P
        r_min = 0 if A[k + 1] > f else 1
        total += max(0, r_max - r_min + 1)
    return total


def list_pieces(V, closed, A, P, f):
    """The pieces of one dashed list: a list of float32 [k, 2] arrays. V: float32 [n, 2]."""
    n = len(V)
    S = prefix_lengths(V, closed)
    m = len(S) - 1
    T = S[m]
    out = []
    if m == 0 or T == 0:
        return out
    cur = [0]  # the largest i < m with S_i <= c for the last c asked; c never decreases

    def segment_of(c):
        i = cur[0]
        while i + 1 < m and S[i + 1] <= c:
            i += 1
        cur[0] = i
        return i

    def snap(c):
        i = segment_of(c)
        if c - S[i] <= SNAP:
            return S[i]
        if S[i + 1] - c <= SNAP:
            return S[i + 1]
        return c

    def point(i, c):  # strictly inside segment i
        t = f32(float(c - S[i]) / float(S[i + 1] - S[i]))
        a, b = V[i], V[(i + 1) % n]
        return (f32(a[0] + f32(f32(b[0] - a[0]) * t)), f32(a[1] + f32(f32(b[1] - a[1]) * t)))

    r = 0
    while r * P - f < T:
        for k in range(0, len(A) - 1, 2):
            a, b = r * P + A[k] - f, r * P + A[k + 1] - f
            if a >= T or b <= 0 or b <= a:
                continue
            s, e = max(a, 0), min(b, T)
            i_s = segment_of(s)
            s = snap(s)
            e = snap(e)
            if e <= s:
                continue
            piece = []
            # X(s): the vertex with the LARGEST j among S_j == s, else a point inside its segment
            j = i_s
            while j + 1 <= m and S[j + 1] <= s:
                j += 1
            piece.append((V[j % n][0], V[j % n][1]) if S[j] == s else point(j, s))
            j += 1
            while j <= m and S[j] < e:
                piece.append((V[j % n][0], V[j % n][1]))
                j += 1
            # X(e): the vertex with the SMALLEST j among S_j == e (j is the first index with S_j >= e)
            piece.append((V[j % n][0], V[j % n][1]) if S[j] == e else point(j - 1, e))
            out.append(np.array(piece, dtype=f32).reshape(-1, 2))
        r += 1
    return out


def dash(poly, subs, sub_draw, dashes, pattern):
    """The whole call. Returns (status, poly float32 [N, 2], subpaths, subpath_draw uint32, subpath_src uint32); arrays are empty
    unless status is OK."""
    empty = (np.zeros((0, 2), f32), np.zeros(0, subpath_dtype), np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    poly = np.asarray(poly, dtype=f32).reshape(-1, 2)
    if validate(dashes, pattern) != OK or any(int(d) >= len(dashes) for d in sub_draw):
        return (E_INVALID_ARG,) + empty
    pats = [pattern_of(r, pattern) for r in dashes]
    lists, draws, srcs, flags = [], [], [], []
    try:
        # the call's "on" intervals, one per undashed list included, before any of them is walked
        budget = 0
        for l, sp in enumerate(subs):
            f0, n, fl = int(sp["first_vertex"]), int(sp["num_vertices"]), int(sp["flags"])
            A, P, f = pats[int(sub_draw[l])]
            budget += 1 if P == 0 else interval_count(A, P, f, prefix_lengths(poly[f0:f0 + n], bool(fl & 1))[-1])
        if budget > MAX_INTERVALS:
            raise Range()
        for l, sp in enumerate(subs):
            f0, n, fl = int(sp["first_vertex"]), int(sp["num_vertices"]), int(sp["flags"])
            V = poly[f0:f0 + n]
            A, P, f = pats[int(sub_draw[l])]
            if P == 0:
                got, gfl = [V.copy()], [fl]
            else:
                got = list_pieces(V, bool(fl & 1), A, P, f)
                gfl = [0] * len(got)
            lists += got
            flags += gfl
            draws += [int(sub_draw[l])] * len(got)
            srcs += [l] * len(got)
    except Range:
        return (E_RANGE,) + empty
    out_subs = np.zeros(len(lists), subpath_dtype)
    counts = np.array([len(p) for p in lists], dtype=np.uint64)
    out_subs["num_vertices"] = counts
    out_subs["first_vertex"] = np.cumsum(counts) - counts
    out_subs["flags"] = flags
    out_poly = np.concatenate(lists).astype(f32) if lists else np.zeros((0, 2), f32)
    return OK, out_poly.reshape(-1, 2), out_subs, np.array(draws, np.uint32), np.array(srcs, np.uint32)
