"""`_lib.launch` -- the one call that owns device, stream and error check of a launch -- against a fake library and patched
torch.cuda functions: no device, no shared library.  What is pinned: the entry point gets the given arguments and then
the current stream of the tensor's device; a tensor on the current device never touches `set_device`; a tensor on another
device has its device current for the call and the caller's back afterwards -- also when the entry point fails or raises
-- and nothing of one call survives into the next."""
import ctypes
import types

import pytest
import torch

from torch_em_amd import _lib


class _FakeLib:
    """tem_x returns `rc` (or raises `exc`) and records its arguments; tem_last_error is the library's message"""

    def __init__(self, events, rc=0, exc=None, msg=b"the library's message"):
        self.events, self.rc, self.exc, self.msg = events, rc, exc, msg

    def tem_x(self, *args):
        self.events.append(("call", args))
        if self.exc is not None:
            raise self.exc
        return self.rc

    def tem_last_error(self):
        return self.msg


class _On:
    """anything with a `.device`"""

    def __init__(self, index):
        self.device = types.SimpleNamespace(type="cuda", index=index)


@pytest.fixture
def world(monkeypatch):
    """-> (events, install): torch.cuda with device 0 current and one stream per device; install(**kw) puts a _FakeLib in"""
    events = []
    state = {"cur": 0}

    def set_device(idx):
        events.append(("set_device", idx))
        state["cur"] = idx

    def current_stream(device=None):
        idx = state["cur"] if device is None or device.index is None else device.index
        return types.SimpleNamespace(cuda_stream=0x1000 + idx)

    monkeypatch.setattr(torch.cuda, "current_device", lambda: state["cur"])
    monkeypatch.setattr(torch.cuda, "set_device", set_device)
    monkeypatch.setattr(torch.cuda, "current_stream", current_stream)

    def install(**kw):
        monkeypatch.setattr(_lib, "_lib", _FakeLib(events, **kw))
    return events, install


def _switches(events):
    return [e for e in events if e[0] == "set_device"]


def test_arguments_then_the_stream_of_the_tensors_device(world):
    events, install = world
    install()
    assert _lib.launch("tem_x", _On(1), 7, None, 2.5) is None
    (args,) = [e[1] for e in events if e[0] == "call"]
    assert args[:3] == (7, None, 2.5) and len(args) == 4
    assert isinstance(args[3], ctypes.c_void_p) and args[3].value == 0x1001   # device 1's stream, not the current device's


def test_same_device_never_sets_the_device(world):
    events, install = world
    install()
    _lib.launch("tem_x", _On(0), 1)
    assert [e[0] for e in events] == ["call"] and events[0][1][1].value == 0x1000


def test_a_device_without_an_index_takes_the_same_device_path(world):
    events, install = world
    install()
    _lib.launch("tem_x", _On(None), 1)
    assert _switches(events) == [] and events[0][1][1].value == 0x1000


def _other_device_order(events):
    """the other-device launch: set_device(1), the call, set_device(0), nothing else"""
    assert [e[0] for e in events] == ["set_device", "call", "set_device"], events
    assert events[0] == ("set_device", 1) and events[2] == ("set_device", 0)


def test_other_device_is_current_for_the_call_only(world):
    events, install = world
    install()
    _lib.launch("tem_x", _On(1), 1)
    _other_device_order(events)
    assert torch.cuda.current_device() == 0


def test_other_device_invalid_argument_restores_and_raises_value_error(world):
    events, install = world
    install(rc=-1)
    with pytest.raises(ValueError) as e:
        _lib.launch("tem_x", _On(1), 1)
    assert str(e.value) == "the library's message"
    _other_device_order(events)
    install(rc=-1, msg=b"")
    with pytest.raises(ValueError) as e:
        _lib.launch("tem_x", _On(0), 1)
    assert str(e.value) == "tem_x: invalid argument"


def test_other_device_runtime_failure_restores_and_raises_tem_error(world):
    events, install = world
    install(rc=-3)
    with pytest.raises(_lib.TemError) as e:
        _lib.launch("tem_x", _On(1), 1)
    assert str(e.value) == "tem_x: the library's message (rc=-3)"
    _other_device_order(events)


def test_other_device_restores_when_the_entry_point_itself_raises(world):
    events, install = world
    install(exc=ctypes.ArgumentError("argument 2: wrong type"))
    with pytest.raises(ctypes.ArgumentError):
        _lib.launch("tem_x", _On(1), 1)
    _other_device_order(events)
    assert torch.cuda.current_device() == 0


def test_no_state_between_calls(world):
    events, install = world
    install(exc=ctypes.ArgumentError("argument 2: wrong type"))
    with pytest.raises(ctypes.ArgumentError):
        _lib.launch("tem_x", _On(1), 1)
    del events[:]
    install()
    _lib.launch("tem_x", _On(0), 1)
    _lib.check(0, "tem_y")
    with pytest.raises(ValueError):
        _lib.check(-1, "tem_y")
    assert _switches(events) == [] and [e[0] for e in events] == ["call"]


def test_ptr():
    assert _lib.ptr(None) is None
    p = _lib.ptr(torch.zeros(4))
    assert isinstance(p, ctypes.c_void_p) and p.value
