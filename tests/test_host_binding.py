"""`_native.call` / `as_c`: the one way from Python into libgpd.so, on entries that return before any launch.  No GPU needed."""
import ctypes

import pytest
import torch


@pytest.fixture(scope="module")
def native():
    from gym_pybullet_drones_amd import _native
    _native.build()
    _native.lib()
    return _native


def _nominal():
    from gym_pybullet_drones_amd.params import DroneParams
    from gym_pybullet_drones_amd.utils.enums import DroneModel
    return DroneParams(DroneModel.CF2X).to_struct(pid_model=DroneModel.CF2X)


def test_as_c_converts_tensors_and_structs_and_nothing_else(native):
    t = torch.zeros(8)
    assert isinstance(native.as_c(t), ctypes.c_void_p) and native.as_c(t).value == t.data_ptr()
    assert native.as_c(t[1:]).value == t.data_ptr() + 4
    P = _nominal()
    ref = native.as_c(P)
    assert type(ref).__name__ == "CArgObject" and ctypes.addressof(ref._obj) == ctypes.addressof(P)
    arr, ptr = (ctypes.c_float * 4)(), ctypes.c_void_p(64)
    for x in (None, 3, 0.5, arr, ptr):
        assert native.as_c(x) is x


def test_call_without_a_stream_fills_an_out_argument(native):
    size = ctypes.c_int32()
    assert native.call("gpd_sizeof_mrac", None, native.NO_STREAM, size) == 0
    assert size.value == ctypes.sizeof(native.GpdMrac)


def test_call_raises_with_the_library_text_and_the_entry_name_unless_allowed(native):
    P, rows = _nominal(), torch.zeros(19 * 128)
    args = ("gpd_plant_derive", None, None, P, None, None, 2, 64, 128, rows)        # a NULL scale table, the NULL stream
    with pytest.raises(native.GpdError) as e:
        native.call(*args)
    msg = str(e.value)
    assert msg.startswith(f"gpd_plant_derive failed (code {native.GPD_EINVAL}): gpd_plant_derive:") and "NULL" in msg   # None arrived as NULL
    assert native.call(*args, allow=(native.GPD_EINVAL,)) == native.GPD_EINVAL
    with pytest.raises(native.GpdError):                   # another code than the one that came back is allowed: still an error
        native.call(*args, allow=(native.GPD_ENOTSUP,))
    with pytest.raises(native.GpdError, match=r"^the plant table failed \(code -1\): gpd_plant_derive"):
        native.call(*args, what="the plant table")


def test_call_passes_a_tensor_as_its_address(native):
    P, scales, rows = _nominal(), torch.zeros(9 * 128), torch.zeros(19 * 128 + 4)
    assert scales.data_ptr() % 16 == 0 and rows.data_ptr() % 16 == 0
    # `rows` four bytes past an aligned address: the entry's alignment check sees exactly that address (and a non-NULL `scales`)
    with pytest.raises(native.GpdError, match="16-byte"):
        native.call("gpd_plant_derive", None, None, P, scales, None, 2, 64, 128, rows[1:])
    with pytest.raises(native.GpdError, match="ld <"):     # aligned: the same call gets past that check to the next one that fails
        native.call("gpd_plant_derive", None, None, P, scales, None, 2, 64, 127, rows)


def test_call_passes_a_struct_by_reference_through_a_void_pointer_parameter(native):
    """gpd_rollout_policy declares its policy as `void *`: ctypes would refuse a Structure there; `call` hands over a reference, and the
    entry reads the struct's members (it objects to `hidden`, the last check before the launch that this state can reach)."""
    from gym_pybullet_drones_amd.policy import GpdPolicy
    P, buf = _nominal(), torch.zeros(13 * 128)
    base = buf.data_ptr()
    st = native.GpdState(kin=base, last_rpm=base, step_counter=base, ld=128)
    cfg = native.GpdStepCfg(num_envs=128, drones_per_env=1, act_type=0, substeps=1, physics_flags=0, pyb_dt=1 / 240, ctrl_dt=1 / 240,
                            inv_ctrl_dt=240.0, lanes_per_wave=64, task=0, trunc_counter=1920)
    pol = GpdPolicy(w1=base, b1=base, w2=base, b2=base, w3=base, b3=base, in_dim=12, hidden=63, activation=0)
    with pytest.raises(native.GpdError, match="gpd_rollout_policy: hidden must be 64"):
        native.call("gpd_rollout_policy", None, None, P, st, cfg, pol, 4, buf, None, None, None, buf, 0, buf, buf, buf, 0, None, None, None, None)


def test_device_guard_is_a_no_op_without_a_device(native):
    assert native.device_guard(None) is native.device_guard(None)
    with native.device_guard(None):
        pass
