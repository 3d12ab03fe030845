"""Rounding to the device's 16-bit matrix types, shared by the restated references of the matrix modes (oracle/gru.py,
oracle/mlp_head.py).  Test infrastructure only."""


def mround(t, mtype):
    """float64 tensor -> the value the device holds after rounding its fp32 copy to `mtype` (None: unchanged)."""
    if mtype is None:
        return t
    return t.float().to(mtype).double()
