"""A plain model of the depression hierarchy, written from the definition: the sweep over the nodes in
ascending key with a union-find, every bowl's region kept as the list of its component's nodes and summed when the bowl spills.
Python integers throughout; the kernels go another way (catchments, a spanning forest, a walk up the parent chain)."""
import numpy as np

from fill_model import NONE, neighbours, outlets

BOWL = np.dtype([("weight", "<u8"), ("volume", "<u8"), ("count", "<u4"), ("own_count", "<u4"), ("floor_at", "<i4"),
                 ("floor_level", "<i4"), ("born_at", "<i4"), ("born_level", "<i4"), ("spill_at", "<i4"), ("spill_level", "<i4"),
                 ("parent", "<i4"), ("n_children", "<u4"), ("n_leaves", "<u4"), ("reserved", "<u4")])


class _Comp:
    """One component of the nodes taken so far: its nodes, whether it holds the outside, and its current bowl while closed."""
    __slots__ = ("nodes", "open", "bowl", "floor", "leaves")

    def __init__(self, nodes, open_, bowl, floor, leaves):
        self.nodes, self.open, self.bowl, self.floor, self.leaves = nodes, open_, bowl, floor, leaves


def bowls(z, conn=8, wrap=False, edge_outlets=True, table=None, invert=False, row_weight=None):
    """((n,) BOWL, (rows, cols) int32 labels) of the lattice z."""
    z = np.asarray(z)
    rows, cols = z.shape
    sign = -1 if invert else 1
    zz = [sign * int(v) for v in z.reshape(-1)]                   # the heights the sweep sees
    out = outlets(rows, cols, wrap, edge_outlets, table).reshape(-1).tolist()
    w_of = [1 if row_weight is None else int(row_weight[i]) for i in range(rows)]
    order = sorted(range(rows * cols), key=lambda v: (zz[v], v))
    comp = {}                                                    # node -> its component's representative node
    comps = {}                                                   # representative -> _Comp
    label = [-1] * (rows * cols)
    recs = []

    def find(v):
        r = v
        while comp[r] != r:
            r = comp[r]
        while comp[v] != r:
            comp[v], v = r, comp[v]
        return r

    def spill(c, v, parent):
        """The current bowl of the closed component c spills at v: its region is c's nodes as they stand."""
        b = recs[c.bowl]
        level = zz[v]
        b["spill_at"], b["spill_level"], b["parent"] = v, level, parent
        b["count"] = len(c.nodes)
        b["weight"] = sum(w_of[n // cols] for n in c.nodes)
        b["volume"] = sum(w_of[n // cols] * (level - zz[n]) for n in c.nodes)
        b["floor_at"], b["n_leaves"] = c.floor[1], c.leaves

    for v in order:
        near = []
        for a, b in neighbours(v // cols, v % cols, rows, cols, conn, wrap):
            u = a * cols + b
            if u in comp:
                r = find(u)
                if r not in near:
                    near.append(r)
        cs = [comps.pop(r) for r in near]
        is_open = out[v] or any(c.open for c in cs)
        closed = [c for c in cs if not c.open]
        if not cs and not out[v]:                                # a leaf is born
            recs.append(dict(born_at=v, born_level=zz[v], spill_at=-1, spill_level=NONE, parent=-1, n_children=0, own_count=0))
            new = _Comp([v], False, len(recs) - 1, (zz[v], v), 1)
        elif len(cs) == 1 and not is_open:                       # v joins the one closed component's current bowl
            new = cs[0]
            new.nodes.append(v)
        elif not is_open:                                        # two or more, all closed: a meta bowl is born
            recs.append(dict(born_at=v, born_level=zz[v], spill_at=-1, spill_level=NONE, parent=-1, n_children=len(cs), own_count=0))
            for c in cs:
                spill(c, v, len(recs) - 1)
            cs.sort(key=lambda c: -len(c.nodes))
            nodes = cs[0].nodes
            for c in cs[1:]:
                nodes.extend(c.nodes)
            nodes.append(v)
            new = _Comp(nodes, False, len(recs) - 1, min(c.floor for c in cs), sum(c.leaves for c in cs))
        else:                                                    # the union is open
            for c in closed:
                spill(c, v, -1)
            new = _Comp(None, True, -1, None, 0)
        comp[v] = v
        for r in near:
            comp[r] = v
        comps[v] = new
        if not new.open:
            label[v] = new.bowl
            recs[new.bowl]["own_count"] += 1
    for c in comps.values():                                     # what never spilled
        if not c.open:
            b = recs[c.bowl]
            b["count"], b["weight"], b["volume"] = len(c.nodes), sum(w_of[n // cols] for n in c.nodes), 0
            b["floor_at"], b["n_leaves"] = c.floor[1], c.leaves
    table_ = np.zeros(len(recs), BOWL)
    for k, b in enumerate(recs):
        spilled = b["spill_at"] >= 0
        table_[k] = (b["weight"] % 2 ** 64, b["volume"] % 2 ** 64, b["count"], b["own_count"], b["floor_at"],
                     sign * zz[b["floor_at"]], b["born_at"], sign * b["born_level"], b["spill_at"],
                     sign * b["spill_level"] if spilled else sign * NONE, b["parent"], b["n_children"], b["n_leaves"], 0)
    return table_, np.array(label, np.int32).reshape(rows, cols)
