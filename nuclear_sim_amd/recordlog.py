"""The host side of a record log ("One record log"): the maintenance event log, the episode records and the event windows
each keep a uint32 cursor on the device, a capacity and record columns the device fills slot by slot (csrc/npd_record_log.h), counting
what does not fit.  Here: the columns with their pinned twins, and the one drain.  Plain dicts; what a log does with its records --
the dtype view, the sort, the derived columns -- stays in its own method of ``BatchedPlantEnv``."""
import numpy as np
import torch

from . import _lib


def allocate(device, capacity: int, columns=()) -> dict:
    """A log of ``capacity`` records: ``columns`` is a list of ``(name, shape, dtype, slot_axis)`` (``add_column``).  Returns ``dev`` and
    ``host`` (name -> tensor), ``slot_axis`` (name -> 0 or -1), ``cursor`` (device, zero), ``host_cursor`` (pinned) and ``capacity``."""
    with torch.cuda.device(device):
        cursor = torch.zeros(1, dtype=torch.int32, device=device)     # a uint32 on the device
    log = {"dev": {}, "host": {}, "slot_axis": {}, "cursor": cursor, "host_cursor": torch.empty(1, dtype=torch.int32, pin_memory=True),
           "capacity": capacity}
    for column in columns:
        add_column(log, *column)
    return log


def add_column(log: dict, name: str, shape, dtype, slot_axis: int = 0) -> torch.Tensor:
    """One more record column, zeroed on the device, with the drain's landing place: pinned host memory, so that a drain is a DMA copy
    rather than a staged one.  ``slot_axis`` (0 or -1) is the axis of ``shape`` the slot indexes.  Returns the device tensor."""
    assert slot_axis in (0, -1), slot_axis
    device = log["cursor"].device
    with torch.cuda.device(device):
        log["dev"][name] = torch.zeros(shape, dtype=dtype, device=device)
    log["host"][name] = torch.empty(shape, dtype=dtype, pin_memory=True)
    log["slot_axis"][name] = slot_axis
    return log["dev"][name]


def drop_column(log: dict, name: str) -> None:
    del log["dev"][name], log["host"][name], log["slot_axis"][name]


def drain(log: dict, device, name: str, noun: str, enable: str, clear: bool = True, allow_overflow: bool = False) -> dict:
    """Read the log back on ``device``'s current stream: numpy copies of the first ``min(count, capacity)`` records of every column, the
    slot axis in front, in the device's order.  A count past the capacity raises and leaves the log as it is -- cursor, columns, nothing
    copied -- unless ``allow_overflow``.  ``clear`` zeroes the cursor.  ``name``, ``noun`` and ``enable`` are the refusal's words."""
    stream = torch.cuda.current_stream(device)
    log["host_cursor"].copy_(log["cursor"], non_blocking=True)
    stream.synchronize()
    count = int(log["host_cursor"][0]) & 0xFFFFFFFF
    cap = log["capacity"]
    if count > cap and not allow_overflow:
        raise _lib.NpbError("%s overflowed: %d %s, capacity %d, %d dropped (%s with a larger capacity, drain more often, or pass "
                            "allow_overflow=True)" % (name, count, noun, cap, count - cap, enable))
    m = min(count, cap)
    if m:
        for column, t in log["dev"].items():
            axis = log["slot_axis"][column]
            log["host"][column].narrow(axis, 0, m).copy_(t.narrow(axis, 0, m), non_blocking=True)
        stream.synchronize()
    out = {column: np.moveaxis(t.numpy(), log["slot_axis"][column], 0)[:m].copy() for column, t in log["host"].items()}
    if clear:
        log["cursor"].zero_()
    return out
