"""The contract the kernels are reached through in a host that owns the stream (pba_ctx_set_stream; include/pba.h: "Streams";
DESIGN §3.3): what tests/test_gpu_caller_stream.py runs and tests/test_caller_stream_cpu.py judges without a GPU.

  HANDOFFS      every entry point of include/pba.h that takes a device pointer (a parameter named d_*), keyed by its C name:
                which parameters they are, whether the call reads or writes the caller's buffer, and the poison the buffer holds
                while its producer is still pending on the stream -- always a VALID input with another answer, so that a broken
                ordering shows as wrong bytes and never as a wild address
  on_stream     the ctx on a caller's stream for the length of a with-block, and back on its own whatever happens inside
  DelayedLib    ctx.lib with a delay in front of every pba_* call

No GPU is touched at import."""
import contextlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PBA_H = os.path.join(ROOT, "include", "pba.h")

SEQ_LENGTHS = (0, 1, 15, 16, 33)          # empty, sub-byte, the dword edge on both sides, a second 16-byte granule
RESPLIT_LENGTHS = (33, 16, 15, 1, 0)      # another split of the same total: the poison of d_offsets_u64
INDEX_TEXT_LEN, INDEX_PARTS = 2000, 3


class Handoff:
    """params: the d_* parameters; role: "reads" (the pending producer is the copy of the real input over the poison) or
    "writes" / "in_place" (the pending producer is the caller's own fill of the buffer: all-ones for "writes", the real
    entries over all-ones for "in_place"); poison: what every d_* buffer holds before that producer has run."""

    def __init__(self, params, role, poison):
        self.params, self.role, self.poison = tuple(params), role, dict(poison)


HANDOFFS = {
    "pba_seqs_from_device_text": Handoff(("d_text", "d_offsets_u64"), "reads",
                                         {"d_text": "'A' * total", "d_offsets_u64": "the offsets of RESPLIT_LENGTHS"}),
    "pba_seqs_export": Handoff(("d_dst",), "writes", {"d_dst": "zero bytes, then the caller's pending 0xFF fill"}),
    "pba_seqs_from_device_packed": Handoff(("d_packed",), "reads", {"d_packed": "zero bytes (every base an A)"}),
    "pba_index_scan": Handoff(("d_entries",), "writes", {"d_entries": "zero bytes, then the caller's pending all-ones fill"}),
    "pba_index_from_entries": Handoff(("d_entries",), "reads", {"d_entries": "all-ones (padding: an empty index)"}),
    "pba_overlap_probes": Handoff(("d_entries",), "writes", {"d_entries": "zero bytes, then the caller's pending all-ones fill"}),
    "pba_overlap_all_probes": Handoff(("d_probe_entries",), "reads", {"d_probe_entries": "all-ones (padding: no probe, no overlap)"}),
    "pba_probe_table_create": Handoff(("d_probe_entries",), "reads", {"d_probe_entries": "all-ones (padding: an empty table)"}),
    "pba_census_mask_probes": Handoff(("d_entries",), "in_place", {"d_entries": "all-ones (padding: nothing to mask)"}),
}

_DECL = re.compile(r"\b(pba_\w+)\s*\(([^;{}]*?)\)\s*;", re.S)
_D_PARAM = re.compile(r"\b(d_\w+)\s*(?:,|$)")


def device_pointer_entry_points(header_text: str) -> dict:
    """{function: (its parameters named d_*, in order)} of every declaration in a header's text that has one.  Comments are
    taken out first: they speak of d_* buffers too."""
    code = re.sub(r"/\*.*?\*/", " ", header_text, flags=re.S)
    code = re.sub(r"//[^\n]*", " ", code)
    out = {}
    for name, params in _DECL.findall(code):
        ds = tuple(m.group(1) for p in params.split(",") for m in [_D_PARAM.search(p.strip())] if m)
        if ds:
            out[name] = ds
    return out


@contextlib.contextmanager
def on_stream(ctx, stream):
    """the ctx on `stream` (anything with a .cuda_stream handle) inside the block, on its own stream afterwards -- always: the
    suite's ctx lives for the whole session, and a stream left behind would be every later test's"""
    try:
        ctx.set_stream(stream.cuda_stream)
        yield ctx
    finally:
        ctx.set_stream(None)


class _Delayed:
    """one library function behind a delay; argtypes, restype and every other attribute are the real function's"""

    def __init__(self, fn, delay):
        object.__setattr__(self, "_fn", fn)
        object.__setattr__(self, "_delay", delay)

    def __call__(self, *args):
        self._delay()
        return self._fn(*args)

    def __getattr__(self, name):
        return getattr(self._fn, name)

    def __setattr__(self, name, value):
        setattr(self._fn, name, value)


class DelayedLib:
    """A stand-in for ctx.lib: every attribute named pba_* that can be called comes back as a wrapper that calls delay() and
    then the real function with the same arguments; everything else is the library's own."""

    def __init__(self, lib, delay):
        self._lib, self._delay = lib, delay

    def __getattr__(self, name):
        attr = getattr(self._lib, name)
        if name.startswith("pba_") and callable(attr):
            return _Delayed(attr, self._delay)
        return attr


@contextlib.contextmanager
def delayed_lib(ctx, delay):
    """ctx.lib replaced by DelayedLib(ctx.lib, delay) inside the block"""
    real = ctx.lib
    ctx.lib = DelayedLib(real, delay)
    try:
        yield ctx
    finally:
        ctx.lib = real
