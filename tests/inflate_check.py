"""What the device inflate tests share (tests/test_gpu_inflate_edges.py, tests/test_gpu_inflate_matrix.py): the destination
of 0xA5 with guard bytes between the items' ranges, and the comparison of a launch with the judge (inflate_edges.judge)."""
import numpy as np

import inflate_edges as E
import lzma_amd

FILL = 0xA5
STATUS = {E.OK: lzma_amd.OK, E.RESULT: lzma_amd.ERR_RESULT, E.EOF: lzma_amd.ERR_UNEXPECTED_EOF, E.OUT_CAP: lzma_amd.ERR_OUT_CAP}


def filled(n):
    import torch
    t = torch.full((max(n, 1),), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


def layout(specs):
    """[(stream, out_cap, residue)] -> ([(stream, dst_off, dst_cap)], total): nineteen guard bytes and more between ranges"""
    items, at = [], 0
    for data, cap, res in specs:
        at += 19
        at += (res - at) % 16
        items.append((data, at, cap))
        at += cap
    return items, at + 19


def check(items, results, buf, judged, what):
    """status, bytes and input used equal the judge; every byte no good item owns is still FILL, or lies in a failed item's range"""
    got = np.frombuffer(buf, dtype=np.uint8)
    free = np.zeros(len(got), dtype=bool)
    for k, ((data, off, cap), (st, produced, used), (cls, out, want_used)) in enumerate(zip(items, results, judged)):
        assert st == STATUS[cls], (what, k, st, cls)
        if cls == E.OK:
            assert (produced, used) == (len(out), want_used), (what, k)
            assert buf[off:off + produced] == out, (what, k)
            free[off:off + produced] = True
        else:
            assert (produced, used) == (0, 0), (what, k)
            free[off:off + cap] = True
    assert bool(np.all(got[~free] == FILL)), what
