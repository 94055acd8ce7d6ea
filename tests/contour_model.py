"""A plain model of the contour lines, written from DESIGN.md section 3.26 alone: loops over cells and elements in index
order, successors followed with a visited set, in Python integers.  It shares no code with moonrtx_amd/contours.py."""
import numpy as np

VOID = 2 ** 31 - 1
LINE = np.dtype([("first", "<u8"), ("n_vertices", "<u4"), ("level_index", "<i4"), ("level", "<i4"), ("head", "<i4"),
                 ("tail", "<i4"), ("closed", "<u4")])


def other_end(rows, cols, wrap, v, k):
    """The node at the other end of edge 2 v + k, or None where the edge is absent."""
    i, j = divmod(v, cols)
    if k == 0:
        if j + 1 < cols:
            return v + 1
        return i * cols if wrap else None
    return v + cols if i + 1 < rows else None


def crossed(z, rows, cols, wrap, c):
    """The edges crossed at level c, ascending."""
    out = []
    for v in range(rows * cols):
        for k in (0, 1):
            o = other_end(rows, cols, wrap, v, k)
            if o is None or z[v] == VOID or z[o] == VOID:
                continue
            if (z[v] >= c) != (z[o] >= c):
                out.append(2 * v + k)
    return out


def cells(rows, cols, wrap):
    """Every cell as (i, j, (NW, NE, SE, SW))."""
    for i in range(rows - 1):
        for j in range(cols if wrap else cols - 1):
            j1 = (j + 1) % cols
            yield i, j, (i * cols + j, i * cols + j1, (i + 1) * cols + j1, (i + 1) * cols + j)


def sides(corners):
    """The edge ids of a cell's sides N, E, S, W."""
    nw, ne, se, sw = corners
    return (2 * nw, 2 * ne + 1, 2 * sw, 2 * nw + 1)


def successors(z, rows, cols, wrap, c):
    """{entry edge: exit edge} over every void-free cell at level c."""
    succ = {}
    for _, _, corners in cells(rows, cols, wrap):
        h = [z[v] for v in corners]
        if VOID in h:
            continue
        a = [x >= c for x in h]
        e = sides(corners)
        entries = [k for k in range(4) if a[k] and not a[(k + 1) % 4]]
        exits = [k for k in range(4) if not a[k] and a[(k + 1) % 4]]
        assert len(entries) == len(exits) <= 2
        if len(entries) == 1:
            pairs = [(entries[0], exits[0])]
        else:
            centre = sum(h) >= 4 * c - 2
            pairs = [(k, (k + 1) % 4 if centre else (k - 1) % 4) for k in entries]
            assert sorted(t for _, t in pairs) == exits
        for k, t in pairs:
            assert e[k] not in succ
            succ[e[k]] = e[t]
    return succ


def trace(z, levels, wrap=False):
    """(lines (n,) LINE, vertices (m,) int32) of the (rows, cols) heights z at the ascending levels."""
    z2 = np.asarray(z)
    rows, cols = z2.shape
    flat = [int(x) for x in z2.reshape(-1)]
    levels = [int(c) for c in levels]
    assert all(a < b for a, b in zip(levels, levels[1:]))
    found = []                                                      # (head edge, level index, vertices, closed)
    for l, c in enumerate(levels):
        edges = crossed(flat, rows, cols, wrap, c)
        succ = successors(flat, rows, cols, wrap, c)
        here = set(edges)
        assert set(succ) <= here and set(succ.values()) <= here
        assert len(set(succ.values())) == len(succ)                 # a partial injection
        has_pred = set(succ.values())
        visited = set()
        for e in edges:                                             # the open lines, from their starts
            if e in has_pred:
                continue
            line = [e]
            visited.add(e)
            while line[-1] in succ:
                line.append(succ[line[-1]])
                assert line[-1] not in visited
                visited.add(line[-1])
            found.append((e, l, line, 0))
        for e in edges:                                             # the closed ones, from their least element
            if e in visited:
                continue
            line = [e]
            visited.add(e)
            while succ[line[-1]] != e:
                line.append(succ[line[-1]])
                assert line[-1] not in visited
                visited.add(line[-1])
            found.append((e, l, line, 1))
        assert visited == here
    found.sort(key=lambda f: (f[0], f[1]))
    lines = np.zeros(len(found), LINE)
    vertices = []
    for r, (e, l, line, closed) in enumerate(found):
        lines[r] = (len(vertices), len(line), l, levels[l], e, line[-1], closed)
        vertices += line
    return lines, np.array(vertices, np.int32).reshape(-1)


def cell_sides(rows, cols, wrap, z):
    """{edge: [the void-free cells it is a side of]} with a cell as its (i, j)."""
    out = {}
    for i, j, corners in cells(rows, cols, wrap):
        if any(z[v] == VOID for v in corners):
            continue
        for e in sides(corners):
            out.setdefault(e, []).append((i, j))
    return out


def check_identities(z, levels, wrap, lines, vertices):
    """The four identities of section 3.26 on any (lines, vertices), in plain integers."""
    z2 = np.asarray(z)
    rows, cols = z2.shape
    flat = [int(x) for x in z2.reshape(-1)]
    levels = [int(c) for c in levels]
    of = cell_sides(rows, cols, wrap, flat)
    verts = [int(v) for v in vertices]
    assert sum(int(n) for n in lines["n_vertices"]) == len(verts)
    per_level = {l: [] for l in range(len(levels))}
    for r in lines:
        a, n, l = int(r["first"]), int(r["n_vertices"]), int(r["level_index"])
        line = verts[a:a + n]
        assert n >= 1 and levels[l] == int(r["level"]) and line[0] == int(r["head"]) and line[-1] == int(r["tail"])
        per_level[l] += line
        # 2: consecutive vertices, and tail to head of a closed line, are two sides of one void-free cell
        pairs = list(zip(line, line[1:])) + ([(line[-1], line[0])] if r["closed"] else [])
        for p, s in pairs:
            assert p != s and set(of.get(p, [])) & set(of.get(s, [])), (p, s)
        if r["closed"]:
            assert line[0] == min(line)
        else:
            # 3: an open line's ends are sides of fewer than two void-free cells (the one the line lies in, if any)
            assert len(of.get(line[0], [])) < 2 and len(of.get(line[-1], [])) < 2
            # 4: on a void-free lattice without wrap they are border edges
            if not wrap and VOID not in flat:
                for e in (line[0], line[-1]):
                    i, j = divmod(e >> 1, cols)
                    assert (i in (0, rows - 1) and e & 1 == 0) or (j in (0, cols - 1) and e & 1 == 1), e
    # 1: the vertices of a level are exactly its crossed edges, each once
    for l, c in enumerate(levels):
        assert sorted(per_level[l]) == crossed(flat, rows, cols, wrap, c), l
    heads = [(int(r["head"]), int(r["level_index"])) for r in lines]
    assert heads == sorted(heads) and len(set(heads)) == len(heads)
