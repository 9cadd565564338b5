"""GPU tests of the state the Python drivers keep between their kernel calls (core_rt.py, core_rt_lin.py, core_rt_ms_lin.py): the
walk flags of Scene.run's composites are cleared when the run raises, and the Planck tables of the linearized runs reach the thermal
slot as arguments -- Scene.thermal_B is never overwritten.  Both on the scalar N = 8 scene of tests/test_gpu_multisensor_thermal_lin.py
(case scalar_n8: 5 points, 6 layers)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

torch = pytest.importorskip("torch")
from test_gpu_multisensor_lin import _pair  # noqa: E402
from test_gpu_multisensor_thermal_lin import CASES, _sources  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vsm():
    import vsmartmom_jl_amd as v
    v._lib.lib()
    return v


@pytest.fixture(scope="module")
def arch(vsm):
    return vsm.Architectures.GPU(0)


def _scalar_n8(vsm, arch, n_planck=None):
    pol, lt, S, L, levels, _, kw = CASES["scalar_n8"]
    pm, pl, _, _ = _pair(vsm, arch, pol, lt, S, L, np.random.default_rng(9), **kw)
    if n_planck is not None:
        pm.sources = _sources(vsm.host_model, "solar+thermal", L, S, n_planck)
    return pm, pl, levels


@pytest.mark.parametrize("reference_order", [False, True], ids=["grouped", "reference_order"])
def test_scene_run_clears_its_walk_flags_when_it_raises(vsm, arch, monkeypatch, reference_order):
    """postprocessing_vza_ raises once inside Scene.run: afterwards no composite of the scene is flagged sources-only or view-rows
    (a flagged composite hands NaN rows to its next reader), and a second run on the same scene equals a fresh scene's bit for bit."""
    CR = vsm.CoreRT
    monkeypatch.setattr(CR, "REFERENCE_ORDER", reference_order)
    pm, _, _ = _scalar_n8(vsm, arch)
    scene = CR.prepare_scene(pm)
    real, seen = CR.postprocessing_vza_, []

    def raise_once(*args, **kw):
        if seen:
            return real(*args, **kw)
        seen.append([(c._sources_only, c._view_rows) for c in scene._composites])
        raise RuntimeError("raised inside Scene.run")
    monkeypatch.setattr(CR, "postprocessing_vza_", raise_once)
    with pytest.raises(RuntimeError, match="raised inside Scene.run"):
        scene.run()
    # (under REFERENCE_ORDER the flags were up when the exception came: the case the old driver left behind)
    assert all(so is reference_order and (vr is not None) == reference_order for so, vr in seen[0])
    assert scene._composites and all(c._sources_only is False and c._view_rows is None for c in scene._composites)
    R, T = [x.clone() for x in scene.run()]
    Rf, Tf = CR.prepare_scene(pm).run()
    torch.cuda.synchronize()
    assert torch.equal(R, Rf) and torch.equal(T, Tf) and bool(torch.isfinite(R).all())


@pytest.mark.parametrize("driver", ["rt_run_lin", "rt_run_multisensor"])
def test_planck_tables_are_arguments_of_the_slot_walks(vsm, arch, monkeypatch, driver):
    """rt_run_lin and the linearized rt_run_multisensor over ThermalEmission(B_layer, B_layer_dot = two tables), with a spy on the
    walks of the thermal slot (ThermalSlot.walk and its linearized twin SceneLin._thermal_lin_walk): scene.fwd.thermal_B is the same
    tensor at every call, and the table each walk is handed is thermal_B, thermal_B_dot[0], thermal_B_dot[1], each in one unbroken
    run of calls, in the order the driver runs them: rt_run_lin the slot and then the Planck block (one walk each), the multi-sensor
    run the Planck sources of every level first and then the slot (a top pass and one walk per segment each)."""
    CR, CL = vsm.CoreRT, vsm.CoreRTLin
    pm, pl, levels = _scalar_n8(vsm, arch, n_planck=2)
    scenes, calls = [], []
    init, fwd_walk, lin_walk = CL.SceneLin.__init__, CR.ThermalSlot.walk, CL.SceneLin._thermal_lin_walk

    def spy_init(self, *args, **kw):
        init(self, *args, **kw)
        scenes.append(self)

    def spy_fwd(self, mom, comp, first, end, B, after=None):
        calls.append((self.scene, self.scene.thermal_B.data_ptr(), B.data_ptr()))
        return fwd_walk(self, mom, comp, first, end, B, after)

    def spy_lin(self, mom, comp, cl, first, end, B, after_layer=None):
        calls.append((self.fwd, self.fwd.thermal_B.data_ptr(), B.data_ptr()))
        return lin_walk(self, mom, comp, cl, first, end, B, after_layer)
    monkeypatch.setattr(CL.SceneLin, "__init__", spy_init)
    monkeypatch.setattr(CR.ThermalSlot, "walk", spy_fwd)
    monkeypatch.setattr(CL.SceneLin, "_thermal_lin_walk", spy_lin)
    if driver == "rt_run_lin":
        CL.rt_run_lin(pm, pl, 0, 1, 1)
    else:
        CL.rt_run_multisensor(pm, pl, 0, 1, 1, levels)
    assert len(scenes) == 1 and scenes[0].sub0 is None and scenes[0].nPlanck == 2
    sc = scenes[0]
    own, d0, d1 = sc.fwd.thermal_B.data_ptr(), sc.thermal_B_dot[0].data_ptr(), sc.thermal_B_dot[1].data_ptr()
    assert len({own, d0, d1}) == 3
    assert calls and all(fwd is sc.fwd and tb == own for fwd, tb, _ in calls)           # thermal_B was never swapped
    handed = [b for _, _, b in calls]
    runs = [b for i, b in enumerate(handed) if i == 0 or handed[i - 1] != b]
    if driver == "rt_run_lin":
        assert handed == [own, d0, d1]
    else:
        assert runs == [d0, d1, own] and len(handed) > 3
