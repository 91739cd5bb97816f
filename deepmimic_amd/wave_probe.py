"""The probe for the wave-level primitives of the step kernels (libdm_hip.so `dm_wave_probe`, deepmimic_amd/csrc/dm_wave_probe.h): TEST SUPPORT.  One launch of `n_waves`
wavefronts evaluates one primitive of the top of dm_device.h / dm_device_duo.h; every lane reads a row of IN doubles and writes a row of OUT, narrowed to float unless
`f64`.  include/dm_hip.h says what an op reads and writes and which `arg` it takes.  tests/test_wave_primitives.py is the caller; nothing of the product is."""
from __future__ import annotations

from typing import Optional

from .binding import check, vp
from .core import load_library

WAVE = 64
IN, OUT, MASK_CHUNKS = 128, 64, 9       # include/dm_hip.h DM_WAVE_PROBE_IN / _OUT / _MASK_CHUNKS
# include/dm_hip.h DM_WOP_*: the position is the op id
OPS = ("WAVE_SHFL", "LANE_BCAST", "HALF_BCAST", "HALF_BCAST_C", "SHFL_XOR_C", "LANE_SEL", "ROW_SEL_C", "HALF_SEL_C", "CHAIN_KEEP", "ROW_FILE", "BALLOT", "WAVE_SUM",
       "HALF_SUM", "RCP", "RSQRT", "MED3", "WG_UNIT", "GRAM32", "GRAM64", "DUO_GRAM32", "XD_OPERANDS", "XD_BLOCK", "XD_TR_STAGE")


def wave_probe(op, f64: int, n_waves: int, in_ptr: int, out_ptr: int, arg: int = 0, stream: int = 0, device_id: int = 0, lib_path: Optional[str] = None):
    """Raw device pointers (ints) to n_waves x 64 x IN and n_waves x 64 x OUT doubles; `op` a name of OPS or its id.  Asynchronous on the HIP stream `stream`."""
    lib = load_library(lib_path)
    if not hasattr(lib, "dm_wave_probe"):
        raise RuntimeError("libdm_hip: this build has no dm_wave_probe (rebuild with __graft_entry__.build())")
    op_id = OPS.index(op) if isinstance(op, str) else int(op)
    check(lib, lib.dm_wave_probe(int(device_id), op_id, int(arg), int(f64), int(n_waves), vp(in_ptr), vp(out_ptr), vp(stream)))
