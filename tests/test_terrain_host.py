"""The refusals of mrtx_occultation and mrtx_horizon_passes without a GPU: the cases of the GPU tests' lists that the calls
refuse before they look for the displacement map give their own texts, in the calls' order, on a context that has no device;
a good argument set then stops at the missing map with MRTX_E_STATE, which is where the other cases of the lists begin."""
import ctypes as C
from datetime import datetime, timedelta, timezone

import numpy as np
import pytest

import passes_model as pm
import terrain_cases as tc
from moonrtx_amd import _lib
from moonrtx_amd import ephemeris as E

DEV = 1 << 40                   # never dereferenced: a call that got as far as using it would not give -1
E_INVALID, E_STATE = -1, -3


@pytest.fixture
def ctx(native_lib):
    """A context handle; without a GPU mrtx_create stops at its first HIP call but hands the context out."""
    c = C.c_void_p()
    rc = native_lib.mrtx_create(C.byref(_lib.MrtxConfig(0, 16, 16, 0, 1, 0, 0)), C.byref(c))
    assert rc in (0, -2) and c.value
    yield c
    native_lib.mrtx_destroy(c)


def no_map(lib, ctx, rc, st):
    assert rc == E_STATE and st.launches == tc.LAUNCHES
    assert lib.mrtx_last_error(ctx) == b"no displacement map: call mrtx_upload_dem first"


def test_occultation_refusals_come_before_the_displacement_map(native_lib, ctx):
    t0 = datetime(2025, 3, 14, 5, 40, tzinfo=timezone.utc)          # the eclipse of the GPU test, its epochs 60 .. 129
    times = [t0 + timedelta(minutes=2 * k) for k in range(70)]
    sun, earth = E.sun_earth_epochs(times, E.Observer(52.2, 21.0, 0.0))
    far = E.far_sun_epochs(sun, times)
    pts = np.array([[10.0, 20.0], [-60.0, 100.0]])
    out = np.full((2, 70), np.nan, np.float32)
    rc, st = tc.occult_call(native_lib, None, **tc.occult_base(pts, far, earth, out))
    assert rc == E_INVALID and st.launches == tc.LAUNCHES
    cases = tc.occult_refusals(pts, far, earth, out, 10.0, DEV)
    assert sum(not needs_dem for _, needs_dem, _ in cases) == 13 and len(cases) == 43
    for text, needs_dem, kw in cases:
        if needs_dem:
            continue
        rc, st = tc.occult_call(native_lib, ctx, **kw)
        tc.refused(native_lib, ctx, rc, st, text)
        assert np.isnan(out).all(), text
    no_map(native_lib, ctx, *tc.occult_call(native_lib, ctx, **tc.occult_base(pts, far, earth, out)))
    assert np.isnan(out).all()


def test_passes_refusals_come_before_the_displacement_map(native_lib, ctx):
    c = pm.case(16)
    lat, lon, hz, pos = c["lat"][:4], c["lon"][:4], c["hz"][:4], c["pos"]
    out = np.zeros((4, 8), np.float32)

    def call(k, pos, **kw):
        st = _lib.MrtxStats()
        st.launches = tc.LAUNCHES
        return tc.passes_call(native_lib, ctx, k, lat, lon, hz, pos, total=C.c_uint64(0), st=st, **kw), st
    cases = tc.passes_refusals(pos, out, DEV)
    assert sum(not needs_dem for _, needs_dem, _ in cases) == 14 and len(cases) == 19
    for text, needs_dem, kw in cases:
        if needs_dem:
            continue
        rc, st = call(**kw)
        tc.refused(native_lib, ctx, rc, st, text)
    no_map(native_lib, ctx, *call(tc.passes_block(), pos, dev_out=None, host_out=out.ctypes.data, cap=0))
    assert (out == 0.0).all()
