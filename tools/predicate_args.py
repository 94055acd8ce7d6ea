"""The predicate options the map tools share (region_catalogue.py, proximity_map.py, region_outlines.py): --below X, --above X or --between A B
select the nodes of one channel of a saved map, and --window places the map on the DEM."""
import math
import sys

import numpy as np


def add_predicate(ap, prefix="", required=True):
    """--{prefix}below / --{prefix}above / --{prefix}between, exactly one of them (or none when not required)."""
    g = ap.add_mutually_exclusive_group(required=required)
    g.add_argument(f"--{prefix}below", type=float, metavar="X")
    g.add_argument(f"--{prefix}above", type=float, metavar="X")
    g.add_argument(f"--{prefix}between", type=float, nargs=2, metavar=("A", "B"))


def bounds(a, prefix=""):
    """(lo, hi) of the parsed predicate: the nodes with lo <= value <= hi are selected."""
    p = prefix.replace("-", "_")
    below, above, between = (getattr(a, p + k) for k in ("below", "above", "between"))
    return (-math.inf, below) if below is not None else (above, math.inf) if above is not None else tuple(between)


def add_window(ap):
    ap.add_argument("--window", type=int, nargs="+", required=True, metavar="N", help="ROW0 COL0 ROWS COLS [STRIDE [WRAP]] in DEM texels")
    ap.add_argument("--dem-size", type=int, nargs=2, default=(23040, 46080), metavar=("H", "W"), help="the DEM the window counts in")


def load_map(path, w):
    """A saved map as (rows, cols, channels), or exit when it is not the window's."""
    field = np.load(path)
    if field.ndim == 2:
        field = field[:, :, None]
    if field.ndim != 3 or field.shape[:2] != (w["rows"], w["cols"]):
        sys.exit(f"{path} is {field.shape}: the window has {w['rows']} x {w['cols']} nodes")
    return field
