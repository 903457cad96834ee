"""tests/caller_stream_inputs.py judged without a GPU: HANDOFFS names every entry point of include/pba.h that takes a device
pointer and no other, DelayedLib delays the pba_* callables and nothing else, on_stream gives the ctx its own stream back when
its body raises."""
import pytest

import caller_stream_inputs as ci


def header():
    with open(ci.PBA_H) as f:
        return f.read()


def test_every_device_pointer_entry_point_has_a_handoff():
    found = ci.device_pointer_entry_points(header())
    assert set(found) == set(ci.HANDOFFS), (sorted(set(found) - set(ci.HANDOFFS)), sorted(set(ci.HANDOFFS) - set(found)))
    for name, h in ci.HANDOFFS.items():
        assert found[name] == h.params and set(h.poison) == set(h.params), name
        assert h.role in ("reads", "writes", "in_place"), name
    assert set(found) == {"pba_seqs_from_device_text", "pba_seqs_export", "pba_seqs_from_device_packed", "pba_index_scan",
                          "pba_index_from_entries", "pba_overlap_probes", "pba_overlap_all_probes", "pba_probe_table_create",
                          "pba_census_mask_probes"}


def test_a_new_device_pointer_parameter_is_noticed():
    """a d_foo parameter added to a copy of the header's text -- on a new function, and on one that has none today -- is found;
    a d_* in a comment is not"""
    text = header()
    assert "pba_ctx_sync(pba_ctx *ctx);" in text
    for grown in (text + "\nint pba_new_thing(pba_ctx *ctx, const void *d_foo,\n                  uint64_t n);\n",
                  text.replace("pba_ctx_sync(pba_ctx *ctx);", "pba_ctx_sync(pba_ctx *ctx, void *d_foo);")):
        found = ci.device_pointer_entry_points(grown)
        assert set(found) - set(ci.HANDOFFS) in ({"pba_new_thing"}, {"pba_ctx_sync"}) and set(found) != set(ci.HANDOFFS)
    assert ci.device_pointer_entry_points("/* int pba_x(void *d_y); */\n// int pba_z(void *d_w);\nint pba_v(void *p);") == {}
    assert ci.device_pointer_entry_points("int pba_a(const void *d_in, int n, void *d_out);") == {"pba_a": ("d_in", "d_out")}


def test_resplit_is_another_split_of_the_same_total():
    assert sum(ci.SEQ_LENGTHS) == sum(ci.RESPLIT_LENGTHS) and ci.SEQ_LENGTHS != ci.RESPLIT_LENGTHS
    assert len(ci.SEQ_LENGTHS) == len(ci.RESPLIT_LENGTHS)


class StubFn:
    """a callable with a ctypes function's two attributes"""

    def __init__(self, log, name):
        self.log, self.name, self.argtypes, self.restype = log, name, [int, int], int

    def __call__(self, *args):
        self.log.append((self.name, args))
        return sum(args)


class StubLib:
    def __init__(self, log):
        self.pba_add = StubFn(log, "pba_add")
        self.pba_ctx_error = StubFn(log, "pba_ctx_error")
        self.other_call = StubFn(log, "other_call")
        self.pba_constant = 7                    # named pba_*, not callable
        self._name = "libstub"


def test_delayed_lib_delays_the_pba_callables_and_nothing_else():
    log = []
    lib = StubLib(log)
    d = ci.DelayedLib(lib, lambda: log.append("delay"))
    assert d.pba_add(2, 3) == 5 and log == ["delay", ("pba_add", (2, 3))]
    del log[:]
    assert d.other_call(1, 1) == 2 and d.pba_constant == 7 and d._name == "libstub" and log == [("other_call", (1, 1))]
    del log[:]
    assert d.pba_ctx_error() == 0 and log == ["delay", ("pba_ctx_error", ())]
    # the real function's attributes, read and written through the wrapper
    assert d.pba_add.argtypes == [int, int] and d.pba_add.restype is int
    d.pba_add.restype = float
    assert lib.pba_add.restype is float
    with pytest.raises(AttributeError):
        d.pba_missing


class StubCtx:
    def __init__(self):
        self.calls, self.lib = [], "the real lib"

    def set_stream(self, handle):
        self.calls.append(handle)


class StubStream:
    cuda_stream = 0x1234


def test_on_stream_restores_the_stream_when_its_body_raises():
    ctx = StubCtx()
    with ci.on_stream(ctx, StubStream()) as c:
        assert c is ctx and ctx.calls == [0x1234]
    assert ctx.calls == [0x1234, None]
    ctx = StubCtx()
    with pytest.raises(KeyError):
        with ci.on_stream(ctx, StubStream()):
            raise KeyError("inside")
    assert ctx.calls == [0x1234, None]

    class Refusing(StubCtx):
        def set_stream(self, handle):
            super().set_stream(handle)
            if handle is not None:
                raise RuntimeError("refused")
    ctx = Refusing()
    with pytest.raises(RuntimeError):
        with ci.on_stream(ctx, StubStream()):
            raise AssertionError("the body must not run")
    assert ctx.calls == [0x1234, None]


def test_set_stream_refuses_the_default_streams_handle():
    """0 is the legacy default stream's handle and the library's "own stream": refused before the library is asked; None and a
    real handle go through as they are"""
    from pacbioassembly_amd import Context

    class Lib:
        def __init__(self):
            self.seen = []

        def pba_ctx_set_stream(self, h, p):
            self.seen.append(p.value)
            return 0
    c = Context.__new__(Context)
    c.lib, c.h = Lib(), None
    with pytest.raises(ValueError):
        c.set_stream(0)
    assert c.lib.seen == []
    c.set_stream(0x7F00)
    c.set_stream(None)
    assert c.lib.seen == [0x7F00, None]


def test_delayed_lib_scope_restores_the_library_when_its_body_raises():
    ctx = StubCtx()
    with pytest.raises(KeyError):
        with ci.delayed_lib(ctx, lambda: None):
            assert isinstance(ctx.lib, ci.DelayedLib)
            raise KeyError("inside")
    assert ctx.lib == "the real lib"
