"""What every operator module starts from: the stream handle, the argument checks, pointers, local events, the workspace cache."""
import torch

from ..native import check, lib


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """The current HIP stream of the current device as a raw handle.  torch.cuda.current_stream() builds a Stream
    object through several Python layers (~8 us): with ~40 launches per sharded step that alone made the host
    the bottleneck, so the raw accessor is used when this torch has it."""
    if _raw_stream is not None:
        return _raw_stream(torch._C._cuda_getDevice())
    return torch.cuda.current_stream().cuda_stream


def _require_device(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                "idgrec_amd operators run on MI355X only: got a %s tensor. There is no CPU fallback; "
                "move the model and inputs to the GPU (device='cuda')." % t.device)


def _require_ids(*tensors):
    """The raw entry points read ids as contiguous int64 (the reference's batches, trainer.py:27-29): anything else
    would be read past its end."""
    for t in tensors:
        if t.dtype != torch.int64 or not t.is_contiguous():
            raise TypeError("batch ids must be contiguous int64 tensors (got %s, contiguous=%s)" % (t.dtype, t.is_contiguous()))


def _f32c(t, name):
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32 (got %s)" % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def _i64c(t, name):
    if t.dtype != torch.int64:
        t = t.long()
    return t if t.is_contiguous() else t.contiguous()


def _ptr(t):
    return t.data_ptr() if t is not None else None  # ctypes converts int / None for void* parameters


def _cached_ws(cache, key, nbytes, device):
    """cache[key], allocated on first use as `nbytes` (an int or a zero-argument callable) uint8 bytes on `device`."""
    ws = cache.get(key)
    if ws is None:
        ws = cache[key] = torch.empty(int(nbytes() if callable(nbytes) else nbytes), dtype=torch.uint8, device=device)
    return ws


class LocalEvent:
    """A device-local event (idg_event_*): orders two streams of one device without the system-scope fence of a default
    HIP / torch event (see include/idgrec.h).  record / wait take raw stream handles (torch.cuda.Stream.cuda_stream)."""

    __slots__ = ("_h", "_done")

    def __init__(self):
        import ctypes as C

        h = C.c_void_p()
        check(lib.idg_event_create(C.byref(h)), "idg_event_create")
        self._h, self._done = h, C.c_int(0)

    def record(self, stream):
        check(lib.idg_event_record(self._h, stream), "idg_event_record")

    def wait(self, stream):
        """Make `stream` wait for the recorded work."""
        check(lib.idg_stream_wait_event(stream, self._h), "idg_stream_wait_event")

    def synchronize(self):
        """Block the host until the recorded work has completed."""
        check(lib.idg_event_synchronize(self._h), "idg_event_synchronize")

    def query(self):
        import ctypes as C

        check(lib.idg_event_query(self._h, C.byref(self._done)), "idg_event_query")
        return bool(self._done.value)

    def __del__(self):
        try:
            lib.idg_event_destroy(self._h)
        except Exception:  # noqa: BLE001 - interpreter shutdown
            pass


def side_stream(device):
    """A second stream for index-only work, bound to a hardware queue NOW.  HIP multiplexes a process's streams over a
    few hardware queues, binding each at its first use; a side stream first used after other streams have taken theirs
    (a communicator's) can land on the MAIN stream's queue, and its kernels then serialise with the step's (measured:
    +30 us per step).  Engines therefore create theirs at construction — before any communicator exists — and touch it
    once.  (A high-priority stream would have a queue class of its own, but waits between the two classes cost far
    more than they save: measured 0.33 -> 0.91 ms per step.)"""
    s = torch.cuda.Stream(device=device)
    with torch.cuda.stream(s):
        torch.zeros(1, dtype=torch.int32, device=device)
    s.synchronize()
    return s


def _ld(t):
    return int(t.stride(0)) if t.shape[0] > 1 else int(t.shape[1])


def _row_base(t, base_row):
    """Pointer of GLOBAL row 0 of a panel whose first row is global row base_row (never dereferenced below that row)."""
    return None if t is None else t.data_ptr() - 4 * int(base_row) * _ld(t)
