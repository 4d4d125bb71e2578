"""GPU: mf_windows_push / ops.windows_push -- the sliding windows of one step's sessions pushed by one launch -- bit for bit against the torch route
LipWindowPool.push has taken so far (cat of the kept context and the new samples, indexed assignment into the pool), for the overlapping shift, the long push, no
context, chunks that are no multiple of 4, and row lists that are a subset, a single row, the whole pool and more than one launch holds."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu


def _torch_route(buf, rows, new):
    """LipWindowPool.push and .rows for a subset, as they stand (lip_driver.py): returns (the pool afterwards, the pushed windows)"""
    n_new = new.shape[1]
    idx = torch.tensor(rows, device=buf.device)
    win = torch.cat([buf[idx][:, n_new:], new], dim=1)
    after = buf.clone()
    after[idx] = win
    return after, win


def _case(N, n, n_new, m, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, n, generator=g).cuda(), torch.randn(m, n_new, generator=g).cuda()


ROWS = {"subset": (8, [5, 0, 3]), "single": (8, [6]), "all": (8, list(range(8))), "two launches": (70, [69] + list(range(64)))}
# (B, l, r, chunk): n = (2B + l + r) * chunk, n_new = 2B * chunk
SHAPES = {"B=1: n_new 640 < context 6400, the shift overlaps": (1, 10, 10, 320), "B=16: n_new 10240 > context": (16, 10, 10, 320), "no context": (2, 0, 0, 320),
          "chunk 322": (1, 10, 10, 322), "chunk 321, l + r odd: rows and n_new off the 16-byte grid": (1, 3, 2, 321)}


@pytest.mark.parametrize("rows_case", list(ROWS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_windows_push_is_bit_equal_to_the_torch_route(lib_built, shape, rows_case):
    from mere_fusion_amd import ops
    B, l, r, chunk = SHAPES[shape]
    N, rows = ROWS[rows_case]
    n, n_new = (2 * B + l + r) * chunk, 2 * B * chunk
    if shape.startswith("B=1:"):
        assert n_new == 640 and n - n_new == 6400
    buf, new = _case(N, n, n_new, len(rows), 7)
    before = buf.clone()
    want_buf, want_win = _torch_route(buf, rows, new)
    win = ops.windows_push(buf, rows, new)
    assert win.shape == (len(rows), n) and torch.equal(win, want_win) and torch.equal(buf, want_buf)
    rest = [k for k in range(N) if k not in rows]
    if rest:                                                             # rows outside the table: byte for byte what they were
        keep = torch.tensor(rest, device="cuda")
        assert torch.equal(buf[keep].view(torch.int32), before[keep].view(torch.int32))
    out = torch.full((len(rows), n), 3.0, device="cuda")                  # a second push, into a caller's block: the context now holds the first push's samples
    new2 = torch.randn(len(rows), n_new, generator=torch.Generator().manual_seed(8)).cuda()
    want_buf2, want_win2 = _torch_route(buf, rows, new2)
    assert ops.windows_push(buf, rows, new2, out=out) is out and torch.equal(out, want_win2) and torch.equal(buf, want_buf2)


def test_windows_push_refuses_before_anything_is_enqueued(lib_built):
    from mere_fusion_amd import _lib, ops
    buf, new = _case(8, 7040, 640, 3, 1)
    before, win = buf.clone(), torch.full((3, 7040), 5.0, device="cuda")
    for rows, text in (([5, 0, 5], "a row appears twice"), ([5, 0, 8], "rows \\[8\\] are out of range"), ([-1, 0, 3], "rows \\[-1\\] are out of range"),
                       ([], "no rows"), ([1, 2], "new must be contiguous fp32 \\[2, n_new\\]")):
        with pytest.raises(RuntimeError, match="windows_push: " + text):
            ops.windows_push(buf, rows, new, out=win if len(rows) == 3 else None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.windows_push(buf.cpu(), [0, 1, 2], new)
    with pytest.raises(RuntimeError, match="out must be"):
        ops.windows_push(buf, [0, 1, 2], new, out=win[:2])
    # the C entry point itself: the same refusals, and a context that no workgroup's LDS holds
    l = _lib.lib()
    call = lambda rows, n=7040, n_new=640, m=None, n_rows=8: l.mf_windows_push(buf.data_ptr(), n_rows, n, new.data_ptr(), n_new, (C.c_int * len(rows))(*rows),
                                                                                   len(rows) if m is None else m, win.data_ptr(), None)
    for kw, text in ((dict(rows=[5, 0, 5]), b"duplicate row 5"), (dict(rows=[5, 0, 8]), b"out of range"), (dict(rows=[0], m=0), b"at least one row"),
                     (dict(rows=[0], n=7040, n_new=7041), b"n_new"), (dict(rows=[0], n=50000, n_new=1000, n_rows=1), b"too large for the")):
        assert call(**kw) == -1 and text in l.mf_last_error(), kw
    assert l.mf_windows_push(buf.data_ptr(), 8, 7040, new.data_ptr(), 640, (C.c_int * 1)(0), 1, buf.data_ptr() + 7040 * 4, None) == -1 and b"win overlaps buf" in l.mf_last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf, before) and (win == 5.0).all()                # nothing was launched
