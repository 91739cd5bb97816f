"""The probe for the device math helpers (libdm_hip.so `dm_math_probe`, deepmimic_amd/csrc/dm_math_probe.h): TEST SUPPORT.  One launch evaluates one helper of
deepmimic_amd/csrc/dm_math.h on `n` rows of doubles, narrowed to float unless `f64`; include/dm_hip.h says which inputs an op reads and what it writes.
tests/test_math_device.py is the caller; nothing of the product is."""
from __future__ import annotations

from typing import Optional

from .binding import check, vp
from .core import load_library

IN, OUT = 18, 12             # include/dm_hip.h DM_MATH_PROBE_IN / DM_MATH_PROBE_OUT: doubles per row
# include/dm_hip.h DM_MOP_*: the position is the op id
OPS = ("SINCOS", "ROT_Y", "ROT_Z", "NORMALIZE_ANGLE", "QMUL", "QNORMALIZE", "QSTANDARDIZE", "QROT", "QUAT_TO_ROT", "QUAT_TO_ROTVEC", "QUAT_THETA", "QUAT_EXP",
       "EXP_MAP_TO_QUAT", "QUAT_DIFF_MUL", "QSLERP", "CALC_HEADING", "CROSS", "CROSS_ADD", "M3_V3", "TMUL", "M3_M3")


def math_probe(op, f64: int, n: int, in_ptr: int, out_ptr: int, stream: int = 0, device_id: int = 0, lib_path: Optional[str] = None):
    """Raw device pointers (ints) to n x IN and n x OUT doubles; `op` a name of OPS or its id.  Asynchronous on the HIP stream `stream` of `device_id`."""
    lib = load_library(lib_path)
    if not hasattr(lib, "dm_math_probe"):
        raise RuntimeError("libdm_hip: this build has no dm_math_probe (rebuild with __graft_entry__.build())")
    op_id = OPS.index(op) if isinstance(op, str) else int(op)
    check(lib, lib.dm_math_probe(int(device_id), op_id, int(f64), int(n), vp(in_ptr), vp(out_ptr), vp(stream)))
