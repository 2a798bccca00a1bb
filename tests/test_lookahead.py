"""The look-ahead window behind FieldSplitter, ScanStats and PulldownRemover's cleaning (savsr_amd.prepass._LookAhead), on host tensors:
N = 6 frames, frame i filled with i, under every split into pushes of 0, 1, 2 or 3 frames followed by the final take(None, last=True).
Empty pushes make the set of splits endless, so it is cut at two of them: every sequence of pushes of 0 .. 3 frames that sums to 6 and has
at most two empty pushes, anywhere -- before the first frame, between pushes, after the last one, and next to each other."""
import pytest
import torch

from savsr_amd.prepass import _LookAhead

N, FRAME = 6, 4          # frames; samples of a frame


def _compositions(total):
    if total == 0:
        yield ()
    for first in range(1, min(3, total) + 1):
        for rest in _compositions(total - first):
            yield (first,) + rest


def _with_zeros(parts, zeros):
    yield parts
    if zeros:
        for at in range(len(parts) + 1):
            yield from _with_zeros(parts[:at] + (0,) + parts[at:], zeros - 1)


def _splits():
    for parts in _compositions(N):
        yield from _with_zeros(parts, 2)


SPLITS = sorted(set(_splits()))


def _video():
    return torch.arange(N, dtype=torch.uint8).view(N, 1).repeat(1, FRAME)          # one tensor: every push is a slice of a larger one


def _check_range(buf, lo, hi, done, pushed):
    """The range [lo, hi) of `buf` continues the video at frame `done`; its neighbours in the buffer are the video's.  -> frames handed back"""
    got = [int(buf[j, 0]) for j in range(lo, hi)]
    assert got == list(range(done, done + hi - lo)), (got, done)
    assert all(bool((buf[j] == buf[j, 0]).all()) for j in range(lo, hi))
    if got and got[0] > 0:
        assert lo >= 1 and int(buf[lo - 1, 0]) == got[0] - 1          # the frame before the range
    if got and got[-1] + 1 < pushed:
        assert hi < buf.shape[0] and int(buf[hi, 0]) == got[-1] + 1   # the frame after it, where one has been pushed
    return len(got)


@pytest.mark.parametrize("split", SPLITS, ids=lambda s: "-".join(map(str, s)))
def test_every_frame_once_in_order_with_its_neighbours(split):
    video, win = _video(), _LookAhead()
    done = pushed = 0
    for k in split:
        buf, lo, hi = win.take(video[pushed:pushed + k])
        pushed += k
        done += _check_range(buf, lo, hi, done, pushed)
        assert done == max(pushed - 1, 0)                             # all but the newest frame are final
        assert win.held <= max(2, k)
        if win.buf is not None:                                       # copies of its own: no larger than the held frames
            assert win.buf.untyped_storage().nbytes() <= win.held * FRAME * video.element_size()
            assert win.buf.untyped_storage().data_ptr() != video.untyped_storage().data_ptr()
    buf, lo, hi = win.take(None, last=True)
    done += _check_range(buf, lo, hi, done, pushed)
    assert done == N and win.held == 0
    assert win.take(None, last=True) == (None, 0, 0)                  # a second finish gives nothing


def test_one_frame_slice_of_a_larger_tensor_is_copied():
    video, win = _video(), _LookAhead()
    buf, lo, hi = win.take(video[:1])
    assert (lo, hi) == (0, 0) and win.held == 1
    assert win.buf.untyped_storage().nbytes() == FRAME * video.element_size()
    video[0] = 9                                                      # the caller's tensor is the caller's again
    assert int(win.buf[0, 0]) == 0


def test_finish_without_a_push_gives_nothing():
    assert _LookAhead().take(None, last=True) == (None, 0, 0)
    win = _LookAhead()
    win.take(_video()[:0])
    buf, lo, hi = win.take(None, last=True)
    assert hi == lo
