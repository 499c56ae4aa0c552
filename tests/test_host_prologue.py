"""CPU tests of the prologue of the C ABI (csrc/qgd_host.h: ENTER): what every entry point answers to a NULL handle, and
that every exported function is classified -- it enters through the prologue, it is one of the host-only setters and
getters that keep working on a handle whose stream is dead, or it is one of the four with their own handling."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "quantumgatedesign.jl_amd", "csrc")
UNITS = ("qgd_host_alloc.cpp", "qgd_host_eval.cpp", "qgd_host_sens.cpp", "qgd_host_comm.cpp")

# touch no device: fields of the handle (or no handle at all)
HOST_ONLY = {
    "qgd_abi_version", "qgd_last_error", "qgd_set_cost_type", "qgd_set_operator_path", "qgd_get_operator_path",
    "qgd_set_small_path", "qgd_set_lambda_derivatives", "qgd_set_save_every", "qgd_set_timing", "qgd_set_comm_timeout",
    "qgd_comm_info", "qgd_comm_unique_id"}
# creation and destruction: there is no handle yet, a dead stream is destroyed in its own way, no communicator is left to destroy
OWN_HANDLING = {"qgd_create", "qgd_create_csc", "qgd_destroy", "qgd_comm_destroy"}
NO_HANDLE = {"qgd_abi_version", "qgd_comm_unique_id", "qgd_create", "qgd_create_csc"}


def _exported_bodies():
    """name -> body of every function the four host units define at file scope under a qgd_ name."""
    out = {}
    for unit in UNITS:
        text = open(os.path.join(CSRC, unit)).read()
        for m in re.finditer(r"^(?:int|void|const char \*) ?(qgd_[a-z0-9_]+)\(.*?\)\s*(?:\{ .*? \}$|\{\n(.*?)^\})", text, re.M | re.S):
            assert m.group(1) not in out, m.group(1)
            out[m.group(1)] = m.group(2) or m.group(0)
    return out


def test_every_entry_point_is_classified(qgd):
    bodies = _exported_bodies()
    exports = set(qgd._lib.EXPORTS)
    assert set(bodies) == exports, set(bodies) ^ exports
    entering = {name for name, body in bodies.items() if re.search(r"\bENTER\(h\b", body)}
    assert not entering & (HOST_ONLY | OWN_HANDLING), entering & (HOST_ONLY | OWN_HANDLING)
    assert entering | HOST_ONLY | OWN_HANDLING == exports, exports - entering - HOST_ONLY - OWN_HANDLING
    # the steps of the prologue are written out nowhere else
    for name, body in bodies.items():
        if name not in OWN_HANDLING:
            assert "hipSetDevice" not in body and "stream_dead" not in body, name
    for unit in UNITS + ("qgd_host.h", "qgd_host_output.cpp", "qgd_host_windows.cpp"):
        assert "NEED_GRID" not in open(os.path.join(CSRC, unit)).read(), unit


def _arguments(fn, fill):
    """NULL handle, then NULL / 0 (fill = 0) or valid-looking pointers and ones (fill = 1) for the rest."""
    buf = (C.c_double * 64)()
    keep, args = [buf], [None]
    for t in fn.argtypes[1:]:
        if t in (C.c_int32, C.c_size_t, C.c_double):
            args.append(t(fill))
        elif not fill:
            args.append(None)
        elif t is C.c_char_p:
            args.append(b"small_path")
        elif t is C.c_void_p:
            args.append(C.cast(buf, C.c_void_p))
        else:                                   # POINTER(c_void_p / c_size_t / c_int32): a place to write to
            keep.append(t._type_())
            args.append(C.byref(keep[-1]))
    return args, keep


@pytest.mark.parametrize("fill", [0, 1], ids=["null-arguments", "plausible-arguments"])
def test_null_handle_is_an_argument_error(qgd, fill):
    """No entry point dereferences a NULL handle: QGD_ERR_ARGUMENT whether its own argument checks or the prologue catch it."""
    lib = qgd._lib.lib()
    assert lib.qgd_destroy(None) is None
    assert lib.qgd_last_error(None) is not None
    for name in qgd._lib.EXPORTS:
        if name in NO_HANDLE or name in ("qgd_destroy", "qgd_last_error"):
            continue
        fn = getattr(lib, name)
        args, keep = _arguments(fn, fill)
        assert fn(*args) == qgd._lib.QGD_ERR_ARGUMENT, name
