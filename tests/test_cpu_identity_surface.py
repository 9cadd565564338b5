"""CPU tests of the identity surface step (core_rt.NATIVE_IDENTITY_SURFACE): the host rule behind VSM_SURFACE_LAYER_IDENTITY, the
switch, the new entry points in the header and the ctypes table, and the argument checks that launch nothing."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALAR, SPECTRAL, BRDF = 0, 1, 2
IDENTITY = 1


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    return v


def test_identity_only_for_scalar_lambertian_above_m0_without_surface_source(vsm):
    """vsm_surface_layer_flags: a host rule on (surface kind, m, surface source) -- identity for (scalar Lambertian, m >= 1, no
    SurfaceSIF / SurfaceEmission in the scene) and for nothing else."""
    CR, L = vsm.CoreRT, vsm._lib.lib()
    assert (CR.SURFACE_LAMBERTIAN_SCALAR, CR.SURFACE_LAMBERTIAN_SPECTRAL, CR.SURFACE_BRDF) == (SCALAR, SPECTRAL, BRDF)
    assert CR.SURFACE_LAYER_IDENTITY == IDENTITY
    for kind in (SCALAR, SPECTRAL, BRDF, 3, -1):
        for m in range(0, 40):
            for src in (False, True):
                want = IDENTITY if (kind == SCALAR and m >= 1 and not src) else 0
                assert CR.surface_layer_flags(kind, m, src) == want, (kind, m, src)
                assert L.vsm_surface_layer_flags(kind, m, int(src)) == want


def test_switch_default_and_signatures(vsm):
    import inspect
    CR = vsm.CoreRT
    assert CR.NATIVE_IDENTITY_SURFACE is True
    sig = inspect.signature(CR.Scene._run_layers_native)
    assert sig.parameters["keep_native"].default is False      # every other driver: the export at the end of the walk, as before
    assert inspect.signature(CR.create_surface_layer_).parameters["has_surface_source"].default is False
    assert CR.RUN_COUNTERS == ("exports_full", "exports_src", "surface_interactions", "guard_launches")


def test_header_declares_the_new_entry_points(vsm):
    header = open(os.path.join(ROOT, "include", "vsmartmom_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    bound = set(vsm._lib.exported_symbols())
    for base, nargs in (("vsm_run_export_sources", 4), ("vsm_run_export_moment", 4), ("vsm_run_surface", 9)):
        for sfx in ("f64", "f32"):
            mt = re.search(r"\bint\s+%s_%s\s*\(([^;]*?)\)\s*;" % (base, sfx), header, flags=re.S)
            assert mt, (base, sfx)
            assert len(mt.group(1).split(",")) == nargs
            assert "%s_%s" % (base, sfx) in bound
        assert len(vsm._lib._SIGS[base + "_{T}"][1]) == nargs
    for name in ("vsm_run_guard_once", "vsm_run_counters", "vsm_surface_layer_flags"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in bound
    assert re.search(r"VSM_SURFACE_LAYER_IDENTITY\s*=\s*1", header)


def _create(vsm, nm=2):
    """A run of S = 0 points on a dummy workspace (nothing is launched)."""
    L = vsm._lib.lib()
    N, ns = 6, 3
    mu, wt = (C.c_double * N)(*([0.5] * N)), (C.c_double * N)(*([1.0] * N))
    q = vsm._lib.vsm_quad_f64(C.cast(mu, C.c_void_p).value, C.cast(wt, C.c_void_p).value, N, ns, 0, 0.5)
    ws = (C.c_double * 2)()
    run = C.c_void_p()
    rc = L.vsm_run_create_ex_f64(C.byref(q), 0, nm, (C.c_int * nm)(*range(nm)), (C.c_int * nm)(*([-1] * nm)), C.cast(ws, C.c_void_p), 16,
                                 1, C.byref(run))
    assert rc == 0, L.vsm_last_error()
    return run, (mu, wt, ws, q)


def test_argument_checks(vsm):
    """Errors, never a silent fallback: a moment outside the run, null arrays, the wrong float type, the guard flag after an
    import; the counters of a fresh run are zero."""
    L = vsm._lib.lib()
    run, keep = _create(vsm)
    try:
        buf = (C.c_double * 4)()
        p = C.cast(buf, C.c_void_p).value
        cc = vsm._lib.vsm_composite(p, p, p, p, p, p)
        vec = vsm._lib.vsm_composite(None, None, None, None, p, p)
        counts = (C.c_int * 4)(9, 9, 9, 9)
        assert L.vsm_run_counters(run, counts) == 0 and list(counts) == [0, 0, 0, 0]
        assert L.vsm_run_counters(run, None) != 0 and L.vsm_run_counters(None, counts) != 0
        assert L.vsm_run_export_sources_f64(run, 1, C.byref(vec), None) == 0       # (S = 0: nothing is launched)
        assert L.vsm_run_export_sources_f64(run, 2, C.byref(vec), None) != 0
        assert L.vsm_run_export_sources_f64(run, -1, C.byref(vec), None) != 0
        assert L.vsm_run_export_sources_f32(run, 0, C.byref(vec), None) != 0
        assert L.vsm_run_export_moment_f64(run, 0, C.byref(vec), None) != 0         # (the matrices are needed there)
        assert L.vsm_run_export_moment_f64(run, 0, C.byref(cc), None) == 0
        assert L.vsm_run_surface_f64(run, 0, 3, None, 0, 0, C.byref(cc), None, None) != 0   # (no surface layer to interact with)
        assert L.vsm_run_surface_f64(run, 0, 3, None, 1, 0, C.byref(vec), None, None) == 0
        assert L.vsm_run_surface_f64(run, 0, 3, None, 1, 1, C.byref(vec), None, None) != 0
        assert L.vsm_run_surface_f64(run, 5, 3, None, 1, 0, C.byref(vec), None, None) != 0
        assert L.vsm_last_error()
        assert L.vsm_run_guard_once(None) != 0
        assert L.vsm_run_guard_once(run) == 0
        assert L.vsm_run_import_f64(run, (vsm._lib.vsm_composite * 2)(cc, cc), None) == 0
        assert L.vsm_run_guard_once(run) != 0
    finally:
        L.vsm_run_destroy(run)
