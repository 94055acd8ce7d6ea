"""A stand-in for libmoonrt.so that needs no GPU: it answers every name in _lib.SIGNATURES, writes every call down and fills
every output from a generator seeded by the call's ordinal number.  tests/test_lattice_facade_host.py checks the lattice
methods of MoonRT against it, and tools/facade_trace.py writes its record to a file so that two trees can be compared.

    fake = FakeLib()
    monkeypatch.setattr(_lib, "load", lambda: fake)

"Device" allocations are host memory, so the real DeviceBuffer runs against the fake and device outputs can be written and
downloaded.  `fake.script` holds the counts the calls report (n_regions, rings, vertices, lines, bowls, rounds, passes,
visits, pairs; default 0) and `fake.refuse` the (entry point, k) pairs to refuse: the k-th call of that entry point since
reset(), counted from 0.  `fake.log` is the record: ("call", name, {argument: value}) for every library call, with
("alloc", number, bytes, device), ("download", where, bytes), ("upload", where, bytes) and ("free", number) between them.

An argument's value is a scalar, the dict of a struct's fields, or for a pointer "null", "host" or "dev<k>+<offset>" -- with
the CRC32 of the bytes behind it appended where it is an input whose extent follows from the other arguments."""
import ctypes as C
import types
import zlib

import numpy as np

from moonrtx_amd import _lib

E_INVALID = -1
REFUSED = b"refused by the script"

_POINT = 16                 # a (lat, lon) pair of doubles
_EPOCH = 112                # an (m, 14) row of doubles


def _rc(a, s="g"):
    g = getattr(a, s)
    return g.rows * g.cols


def _thermal_out(a):
    rec, nn = max(a.m - a.model.n_spin, 1), max(a.model.n_nodes, 1)
    return {0: 4 * rec, 1: 16, 2: 4 * a.m, 3: 8 * rec, 4: 4 * rec * nn, 5: 16 * nn}[a.mode] * a.n


def _passes_out(a):
    if a.k.mode == _lib.PASSES_FULL:
        return 16 * a.n * a.k.n_sat * a.k.m
    return 32 * a.n if a.k.mode == _lib.PASSES_SUMMARY else _lib.PASS_DTYPE.itemsize * a.cap


_HORIZON = {"dh hh": lambda a: 4 * a.n * a.n_az}
_THERMAL_HEAD = "ctx pts n n_az dh hh ep fl m model mode dx hx x_len"
_THERMAL_IN = {"pts": lambda a: _POINT * a.n, **_HORIZON, "ep": lambda a: _EPOCH * a.m, "fl": lambda a: 8 * a.m,
               "dx hx": lambda a: 4 * a.x_len}

# entry point: (argument names, {input: bytes}, {output: bytes}, {counter argument: script key}); a name pair "d h" is a
# (device, host) pointer pair of one table
SPEC = {
    "mrtx_illum_grid": ("ctx g dev host st", {}, {"dev host": lambda a: 16 * (a.g.row_end - a.g.row_begin) * a.g.w}, {}),
    "mrtx_illum_points": ("ctx pts n n_sun host st", {"pts": lambda a: _POINT * a.n}, {"host": lambda a: 16 * a.n}, {}),
    "mrtx_illum_series": ("ctx pts n ep m first count n_sun dev host st",
                          {"pts": lambda a: _POINT * a.n, "ep": lambda a: _EPOCH * a.m, "first": lambda a: 4 * a.n},
                          {"dev host": lambda a: 16 * a.n * a.count}, {}),
    "mrtx_horizon_points": ("ctx pts n n_az n_bis dev host st", {"pts": lambda a: _POINT * a.n},
                            {"dev host": lambda a: 4 * a.n * a.n_az}, {}),
    "mrtx_horizon_raised": ("ctx pts hts radius_m n n_az n_bis dev host st",
                            {"pts": lambda a: _POINT * a.n, "hts": lambda a: 8 * a.n}, {"dev host": lambda a: 4 * a.n * a.n_az}, {}),
    "mrtx_horizon_sun": ("ctx pts n n_az dh hh ep m mode dev host st",
                         {"pts": lambda a: _POINT * a.n, **_HORIZON, "ep": lambda a: _EPOCH * a.m},
                         {"dev host": lambda a: 4 * a.n * (4 if a.mode else a.m)}, {}),
    "mrtx_horizon_windows": ("ctx pts n n_az dh hh ea eb m min_a min_b dev host st",
                             {"pts": lambda a: _POINT * a.n, **_HORIZON, "ea": lambda a: _EPOCH * a.m, "eb": lambda a: _EPOCH * a.m},
                             {"dev host": lambda a: 32 * a.n}, {}),
    "mrtx_horizon_mask": ("ctx pts n n_az dh hh ea eb m min_a min_b dev host st",
                          {"pts": lambda a: _POINT * a.n, **_HORIZON, "ea": lambda a: _EPOCH * a.m, "eb": lambda a: _EPOCH * a.m},
                          {"dev host": lambda a: 8 * a.n * ((a.m + 63) // 64)}, {}),
    "mrtx_power_budget": ("ctx pts n n_az dh hh ep gen load m md mode dev host st",
                          {"pts": lambda a: _POINT * a.n, **_HORIZON, "ep": lambda a: _EPOCH * a.m, "gen": lambda a: 8 * a.m,
                           "load": lambda a: 8 * a.m}, {"dev host": lambda a: a.n * (64 if a.mode else 4 * a.m)}, {}),
    "mrtx_occultation": ("ctx pts n es eb m mode dev host st",
                         {"pts": lambda a: _POINT * a.n, "es": lambda a: _EPOCH * a.m, "eb": lambda a: _EPOCH * a.m},
                         {"dev host": lambda a: 4 * a.n * (8 if a.mode else a.m)}, {}),
    "mrtx_horizon_passes": ("ctx k pts hts n n_az dh hh pos dev host cap total st",
                            {"pts": lambda a: _POINT * a.n, "hts": lambda a: 8 * a.n, **_HORIZON,
                             "pos": lambda a: 24 * a.k.n_sat * a.k.m}, {"dev host": _passes_out}, {"total": "passes"}),
    "mrtx_thermal": ("ctx pts n n_az dh hh ep fl m model mode dev host st",
                     {k: v for k, v in _THERMAL_IN.items() if k != "dx hx"}, {"dev host": _thermal_out}, {}),
    "mrtx_view_hits": ("ctx pts n k dev host st", {"pts": lambda a: _POINT * a.n}, {"dev host": lambda a: 4 * a.n * (2 * a.k + 1)}, {}),
    "mrtx_scatter_flux": ("ctx ix n k ex_d ex_h length n_hits m albedo_h emissivity dev host st",
                          {"ix": lambda a: 4 * a.n * a.k, "ex_d ex_h": lambda a: 4 * a.length}, {"dev host": lambda a: 4 * a.n * a.m}, {}),
    "mrtx_thermal_scatter": (_THERMAL_HEAD + " dev host st", _THERMAL_IN, {"dev host": _thermal_out}, {}),
    "mrtx_thermal_column": (_THERMAL_HEAD + " sp dev host st", _THERMAL_IN, {"dev host": _thermal_out}, {}),
    "mrtx_thermal_occulted": (_THERMAL_HEAD + " sp es eb dev host st",
                              {**_THERMAL_IN, "es": lambda a: _EPOCH * a.m, "eb": lambda a: _EPOCH * a.m}, {"dev host": _thermal_out}, {}),
    "mrtx_sight_grid": ("ctx g dev host st", {}, {"dev host": lambda a: 4 * (a.g.row_end - a.g.row_begin) * a.g.w}, {}),
    "mrtx_sight_points": ("ctx pts n obs n_obs target_h_m mast_max_m radius_m n_bis dev host st",
                          {"pts": lambda a: _POINT * a.n, "obs": lambda a: 24 * a.n_obs}, {"dev host": lambda a: 4 * a.n}, {}),
    "mrtx_traverse_lengths": ("t H W out", {}, {"out": lambda a: 12 * max(a.t.rows, 1)}, {}),
    "mrtx_traverse": ("ctx t ij cost0 n pen_d pen_h cost_d cost_h pred_d pred_h visits st",
                      {"ij": lambda a: 8 * a.n, "cost0": lambda a: 8 * a.n, "pen_d pen_h": lambda a: 4 * _rc(a, "t")},
                      {"cost_d cost_h": lambda a: 8 * _rc(a, "t"), "pred_d pred_h": lambda a: _rc(a, "t")}, {"visits": "visits"}),
    "mrtx_traverse_timed": ("ctx t tt ij tick0 n pen_d pen_h av_d av_h arr_d arr_h pred_d pred_h visits st",
                            {"ij": lambda a: 8 * a.n, "tick0": lambda a: 8 * a.n, "pen_d pen_h": lambda a: 4 * _rc(a, "t"),
                             "av_d av_h": lambda a: 8 * _rc(a, "t") * ((a.tt.n_epochs + 63) // 64)},
                            {"arr_d arr_h": lambda a: 8 * _rc(a, "t"), "pred_d pred_h": lambda a: _rc(a, "t")}, {"visits": "visits"}),
    "mrtx_traverse_heights": ("ctx t dev host st", {}, {"dev host": lambda a: 4 * _rc(a, "t")}, {}),
    "mrtx_relief": ("ctx t dev host st", {}, {"dev host": lambda a: 16 * _rc(a, "t")}, {}),
    "mrtx_relief_share": ("ctx s tab_d tab_h dev host st", {"tab_d tab_h": lambda a: 16 * _rc(a, "s")},
                          {"dev host": lambda a: 4 * _rc(a, "s")}, {}),
    "mrtx_regions_label": ("ctx r f_d f_h m_d m_h lab_d lab_h n st",
                           {"f_d f_h": lambda a: 4 * _rc(a, "r") * a.r.n_ch, "m_d m_h": lambda a: _rc(a, "r")},
                           {"lab_d lab_h": lambda a: 4 * _rc(a, "r")}, {"n": "n_regions"}),
    "mrtx_regions_stats": ("ctx rows cols wrap lab_d lab_h n w rec_d rec_h st",
                           {"lab_d lab_h": lambda a: 4 * a.rows * a.cols, "w": lambda a: 4 * a.rows}, {"rec_d rec_h": lambda a: 56 * a.n}, {}),
    "mrtx_regions_zonal": ("ctx z lab_d lab_h n f_d f_h w rec_d rec_h hist_d hist_h st",
                           {"lab_d lab_h": lambda a: 4 * _rc(a, "z"), "f_d f_h": lambda a: 4 * _rc(a, "z") * a.z.n_ch,
                            "w": lambda a: 4 * a.z.rows},
                           {"rec_d rec_h": lambda a: 56 * a.n * a.z.n_ch, "hist_d hist_h": lambda a: 8 * a.n * (a.z.n_bins + 2)}, {}),
    "mrtx_regions_shape": ("ctx rows cols wrap connectivity lab_d lab_h n ew ns rec_d rec_h st",
                           {"lab_d lab_h": lambda a: 4 * a.rows * a.cols, "ew": lambda a: 4 * a.rows, "ns": lambda a: 4 * (a.rows + 1)},
                           {"rec_d rec_h": lambda a: 32 * a.n}, {}),
    "mrtx_proximity": ("ctx p pos_d pos_h lab_d lab_h near_d near_h d2_d d2_h pairs st",
                       {"pos_d pos_h": lambda a: 12 * _rc(a, "p"), "lab_d lab_h": lambda a: 4 * _rc(a, "p")},
                       {"near_d near_h": lambda a: 4 * _rc(a, "p"), "d2_d d2_h": lambda a: 8 * _rc(a, "p")}, {"pairs": "pairs"}),
    "mrtx_regions_reach": ("ctx rows cols lab_d lab_h n d2_d d2_h near_d near_h rec_d rec_h st",
                           {"lab_d lab_h": lambda a: 4 * a.rows * a.cols, "d2_d d2_h": lambda a: 8 * a.rows * a.cols,
                            "near_d near_h": lambda a: 4 * a.rows * a.cols}, {"rec_d rec_h": lambda a: 32 * a.n}, {}),
    "mrtx_regions_outline": ("ctx o lab_d lab_h n w ring_d ring_h cap_r vert_d vert_h cap_v nr nv st",
                             {"lab_d lab_h": lambda a: 4 * _rc(a, "o"), "w": lambda a: 4 * a.o.rows},
                             {"ring_d ring_h": lambda a: 48 * a.cap_r, "vert_d vert_h": lambda a: 8 * a.cap_v},
                             {"nr": "rings", "nv": "vertices"}),
    "mrtx_contours": ("ctx k z_d z_h levels line_d line_h cap_l vert_d vert_h cap_v nl nv st",
                      {"z_d z_h": lambda a: 4 * _rc(a, "k"), "levels": lambda a: 4 * a.k.n_levels},
                      {"line_d line_h": lambda a: 32 * a.cap_l, "vert_d vert_h": lambda a: 4 * a.cap_v}, {"nl": "lines", "nv": "vertices"}),
    "mrtx_fill": ("ctx f z_d z_h out_d out_h fill_d fill_h visits st",
                  {"z_d z_h": lambda a: 4 * _rc(a, "f"), "out_d out_h": lambda a: _rc(a, "f")}, {"fill_d fill_h": lambda a: 4 * _rc(a, "f")},
                  {"visits": "visits"}),
    "mrtx_fill_basins": ("ctx rows cols wrap connectivity lab_d lab_h n z_d z_h fill_d fill_h w rec_d rec_h st",
                         {"lab_d lab_h": lambda a: 4 * a.rows * a.cols, "z_d z_h": lambda a: 4 * a.rows * a.cols,
                          "fill_d fill_h": lambda a: 4 * a.rows * a.cols, "w": lambda a: 4 * a.rows}, {"rec_d rec_h": lambda a: 48 * a.n}, {}),
    "mrtx_bowls": ("ctx b z_d z_h out_d out_h w rec_d rec_h cap lab_d lab_h nb rounds st",
                   {"z_d z_h": lambda a: 4 * _rc(a, "b"), "out_d out_h": lambda a: _rc(a, "b"), "w": lambda a: 4 * a.b.rows},
                   {"rec_d rec_h": lambda a: 64 * a.cap, "lab_d lab_h": lambda a: 4 * _rc(a, "b")}, {"nb": "bowls", "rounds": "rounds"}),
}


def _plain(v):
    """A ctypes value as what json can write."""
    if isinstance(v, C.Structure):
        return {name: _plain(getattr(v, name)) for name, _ in v._fields_}
    if isinstance(v, C.Array):
        return [_plain(x) for x in v]
    if isinstance(v, C._SimpleCData):
        return v.value
    if isinstance(v, bytes):
        return v.decode(errors="replace")
    if isinstance(v, (np.integer, np.floating)):
        return v.item()
    return v


class FakeLib:
    def __init__(self):
        self.reset()

    def reset(self):
        """A new scenario: an empty record, no allocations, nothing scripted or refused."""
        self.log, self.allocs, self.script, self.refuse, self.seen, self.error = [], [], {}, set(), {}, b""

    # ---- what the record is read through
    def calls(self, name=None):
        """The (name, arguments) of the recorded library calls, of one entry point if `name` is given."""
        return [(e[1], e[2]) for e in self.log if e[0] == "call" and name in (None, e[1])]

    def live(self):
        """The numbers of the allocations not freed."""
        return [k for k, al in enumerate(self.allocs) if not al["freed"]]

    def where(self, addr):
        if addr is None:
            return "null"
        for k, al in enumerate(self.allocs):
            if al["base"] <= addr < al["base"] + max(al["nbytes"], 1):
                return f"dev{k}+{addr - al['base']}"
        return "host"

    # ---- the entry points
    def __getattr__(self, name):
        if name not in _lib.SIGNATURES:
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _call(self, name, args):
        own = getattr(self, "_" + name, None)
        if own is not None:
            return own(*args)
        if name not in SPEC:                    # renderer entry points: answered, not recorded
            return 0
        names, ins, outs, counters = SPEC[name]
        names = names.split()
        assert len(names) == len(args), f"{name} takes {len(names)} arguments, got {len(args)}"
        a = types.SimpleNamespace(**{k: getattr(v, "_obj", v) for k, v in zip(names, args)})
        pointers = {p for key in list(ins) + list(outs) for p in key.split()}
        rec = {}
        for k in names:
            v = getattr(a, k)
            if k == "ctx" or k == "st" or k in counters:
                continue
            rec[k] = self.where(v) if k in pointers else _plain(v)
        for key, size in ins.items():
            for p in key.split():
                addr = getattr(a, p)
                if addr is not None:
                    rec[p] += f" crc {zlib.crc32(C.string_at(addr, max(int(size(a)), 0))):08x}"
        ordinal = len(self.calls())
        self.log.append(("call", name, rec))
        k = self.seen.get(name, 0)
        self.seen[name] = k + 1
        if (name, k) in self.refuse:
            self.error = REFUSED
            return E_INVALID
        if "pts" in names and a.n < 1:
            self.error = b"n must be >= 1"        # an empty point query, as the library refuses it
            return E_INVALID
        rng = np.random.default_rng(ordinal)
        for key, size in outs.items():
            nbytes = max(int(size(a)), 0)
            for p in key.split():
                addr = getattr(a, p)
                if addr is not None and nbytes:
                    data = np.zeros(nbytes, np.uint8)
                    data[::8] = rng.integers(1, 4, data[::8].size)      # small integers and tiny floats in every number format
                    C.memmove(addr, data.ctypes.data, nbytes)
        for p, key in counters.items():
            getattr(a, p).value = int(self.script.get(key, 0))
        self._vertex_counts(name, a)
        st = getattr(a, "st", None)
        if st is not None:
            st.launches, st.kernel_ms, st.shadow_rays, st.bounce_rays, st.reserved = 1, 0.5 * (ordinal + 1), ordinal, 3, 2
        return 0

    @staticmethod
    def _vertex_counts(name, a):
        """Outlines and Contours check that their records' n_vertices add up to the vertex table: the first record gets all."""
        if name == "mrtx_regions_outline":
            from moonrtx_amd import regions
            addr, cap, n_v, dtype = a.ring_d if a.ring_d is not None else a.ring_h, a.cap_r, a.cap_v, regions.RING_DTYPE
        elif name == "mrtx_contours":
            addr, cap, n_v, dtype = a.line_d if a.line_d is not None else a.line_h, a.cap_l, a.cap_v, _lib.CONTOUR_LINE_DTYPE
        else:
            return
        if addr is not None and cap:
            table = np.frombuffer((C.c_char * (dtype.itemsize * cap)).from_address(addr), dtype)
            table["n_vertices"] = 0
            table["n_vertices"][0] = n_v

    # ---- entry points with a behaviour of their own
    def _mrtx_abi_version(self):
        return _lib.ABI_VERSION

    def _mrtx_create(self, cfg, ctx):
        self.device = cfg._obj.device
        ctx._obj.value = 1
        return 0

    def _mrtx_last_error(self, ctx):
        return self.error

    def _mrtx_get_config(self, ctx, cfg):
        cfg._obj.device = getattr(self, "device", 0)
        return 0

    def _samples(self, name, n, out, ok):
        self.log.append(("call", name, {"n": n, "out": self.where(out)}))
        if n not in ok:
            return E_INVALID
        np.frombuffer((C.c_float * (2 * n)).from_address(out), np.float32)[:] = np.arange(2 * n) / (2 * n)
        return 0

    def _mrtx_illum_sun_samples(self, n, out):
        return self._samples("mrtx_illum_sun_samples", n, out, (1, 2, 4, 8, 16, 32, 64))

    def _mrtx_view_dir_samples(self, k, out):
        return self._samples("mrtx_view_dir_samples", k, out, (16, 32, 64, 128, 256, 512, 1024))

    def _mrtx_relief_scales(self, t, H, W, out):
        """(kx, ky) per row from the script's "scales" = (kx of the first half of the rows, kx of the rest, ky)."""
        t = t._obj
        self.log.append(("call", "mrtx_relief_scales", {"t": _plain(t), "H": H, "W": W, "out": self.where(out)}))
        kx0, kx1, ky = self.script.get("scales", (1.0, 1.0, 1.0))
        rows = max(t.rows, 1)
        table = np.frombuffer((C.c_double * (2 * rows)).from_address(out), np.float64).reshape(rows, 2)
        table[:, 0], table[:, 1] = np.where(np.arange(rows) < rows // 2, kx0, kx1), ky
        return 0

    def _mrtx_dev_alloc(self, device, nbytes, p):
        buf = C.create_string_buffer(max(int(nbytes), 1))
        self.log.append(("alloc", len(self.allocs), int(nbytes), device))
        self.allocs.append({"base": C.addressof(buf), "nbytes": int(nbytes), "buf": buf, "device": device, "freed": False})
        p._obj.value = C.addressof(buf)
        return 0

    def _mrtx_dev_free(self, device, ptr):
        for k, al in enumerate(self.allocs):
            if al["base"] == ptr and not al["freed"]:
                al["freed"] = True          # the memory stays, so that no later allocation takes its address
                self.log.append(("free", k))
        return 0

    def _mrtx_dev_download(self, device, dst, src, nbytes):
        self.log.append(("download", self.where(src), int(nbytes)))
        C.memmove(dst, src, nbytes)
        return 0

    def _mrtx_dev_upload(self, device, dst, src, nbytes):
        self.log.append(("upload", self.where(dst), int(nbytes)))
        C.memmove(dst, src, nbytes)
        return 0
