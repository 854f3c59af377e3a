"""Ray queries with a per-ray tmax (include/rt_mi355x.h: rt_trace_rays[_device]) without a GPU: the exported entry points, the argument
checks in front of the device, the Python wrapper's shape checks, and the ISA hazard scan of the query kernel's unit."""
import ctypes as C

import numpy as np
import pytest

from rtamd import abi, scenes
from rtamd.renderer import Scene


def test_both_libraries_export_the_query_entry_points(rtlib, devlib):
    for lib in (rtlib, devlib):
        for name in ("rt_trace_rays", "rt_trace_rays_device"):
            assert hasattr(lib, name), name
    assert rtlib.rt_abi_version() == 8


def _query(n, mode, org=None, dirs=None, tmax=None, t=None, occ=None):
    q = abi.rt_ray_query(n=n, mode=mode)
    q.org = org.ctypes.data if org is not None else None
    q.dir = dirs.ctypes.data if dirs is not None else None
    q.tmax = tmax.ctypes.data if tmax is not None else None
    q.t = t.ctypes.data if t is not None else None
    q.occluded = occ.ctypes.data if occ is not None else None
    return q


@pytest.mark.parametrize("entry", ["rt_trace_rays", "rt_trace_rays_device"])
def test_argument_checks_come_before_the_device(rtlib, entry):
    """On a host-only scene: RT_ERR_INVALID for a NULL scene, query or required pointer and for an unknown mode, RT_ERR_NO_DEVICE for a
    well-formed query, RT_OK for n == 0 (nothing to launch)."""
    s = Scene(scenes.get_scene("cornell"), device=-1)
    fn = getattr(rtlib, entry)
    call = (lambda h, q: fn(h, q)) if entry == "rt_trace_rays" else (lambda h, q: fn(h, q, None))
    org, dirs = np.zeros((4, 3), np.float32), np.ones((4, 3), np.float32)
    t, occ, tmax = np.zeros(4, np.float32), np.zeros(4, np.uint8), np.ones(4, np.float32)
    C_, A = abi.RT_QUERY_CLOSEST, abi.RT_QUERY_ANY
    q = _query(4, C_, org, dirs, t=t)
    assert call(None, C.byref(q)) == abi.RT_ERR_INVALID
    assert call(s.h, None) == abi.RT_ERR_INVALID
    for bad in (_query(4, C_, None, dirs, t=t), _query(4, C_, org, None, t=t), _query(4, C_, org, dirs),  # no output at all
                _query(4, A, org, dirs, t=t), _query(4, 2, org, dirs, t=t, occ=occ), _query(0, 7)):
        assert call(s.h, C.byref(bad)) == abi.RT_ERR_INVALID
    for good in (_query(4, C_, org, dirs, t=t), _query(4, C_, org, dirs, tmax, t=t), _query(4, A, org, dirs, occ=occ)):
        assert call(s.h, C.byref(good)) == abi.RT_ERR_NO_DEVICE
        assert "host-only" in rtlib.rt_last_error().decode()
    for empty in (_query(0, C_), _query(0, A), _query(0, C_, org, dirs, t=t)):
        assert call(s.h, C.byref(empty)) == abi.RT_OK
    s.close()


def test_python_wrapper(rtlib):
    s = Scene(scenes.get_scene("cube"), device=-1)
    with pytest.raises(abi.RtError) as e:
        s.trace(np.zeros((2, 3)), np.ones((2, 3)), any_hit=True)
    assert e.value.status == abi.RT_ERR_NO_DEVICE
    with pytest.raises(ValueError):
        s.trace(np.zeros((2, 3)), np.ones((3, 3)))
    with pytest.raises(ValueError):
        s.trace(np.zeros((2, 3)), np.ones((2, 3)), tmax=np.ones(3))
    assert s.trace(np.zeros((0, 3)), np.zeros((0, 3)), any_hit=True).shape == (0,)
    with pytest.raises(abi.RtError) as e:
        s.trace_device(5, 0, 0)
    assert e.value.status == abi.RT_ERR_INVALID
    s.close()


def test_query_kernels_pass_the_isa_hazard_scan(tmp_path):
    """k_query<false> and k_query<true> (rt_query.hip) through tests/test_isa_hazards.py's checker: both carry the asm node fetch and
    break none of its rules."""
    from test_denoise import _listing
    from test_isa_hazards import _check
    groups = _check(_listing("rt_query.hip", tmp_path))
    for inst in ("k_queryILb0E", "k_queryILb1E"):
        assert any(inst in k for k in groups), groups
