"""The stand-in for libktf_hip.so that test_runner_launches_cpu.py and test_ops_calls_cpu.py share: every library call is written
out as text instead of launching anything."""

import ctypes as C

STREAM = object()       # what the tests make L.stream_ptr() return


class Recorder:
    """Stands in for the ctypes library: the symbols `host_helpers` (a compiled pattern) matches go to the real one (written to
    `lines` with their result when `log_host`), every other call is written to `lines` and returns 0. `names(address)` gives the
    text of a pointer argument."""

    def __init__(self, real, host_helpers, names=None, log_host=False):
        self.real, self.host_helpers, self.names, self.log_host = real, host_helpers, names, log_host
        self.lines, self.called = [], set()

    def __getattr__(self, name):
        host = self.host_helpers.fullmatch(name)
        if host and not self.log_host:
            return getattr(self.real, name)

        def call(*args):
            self.called.add(name)
            line = f"{name}({', '.join(self.arg(a) for a in args)})"
            res = getattr(self.real, name)(*args) if host else 0
            self.lines.append(f"{line} = {res}" if host else line)
            return res
        return call

    def arg(self, a):
        if a is STREAM:
            return "stream"
        if a is None:
            return "null"
        if isinstance(a, C.c_void_p):
            return self.names(a.value)
        if isinstance(a, bool):
            return str(int(a))
        if isinstance(a, int):
            return str(a)
        if isinstance(a, float):
            return repr(a)
        if type(a).__name__ == "CArgObject" and isinstance(a._obj, C.Structure):
            d = a._obj
            tag = {"TdnnDesc": "desc"}.get(type(d).__name__, type(d).__name__)
            vals = ((f, getattr(d, f)) for f, _ in d._fields_)
            return tag + "{" + " ".join(f"{f}={list(v) if isinstance(v, C.Array) else v}" for f, v in vals) + "}"
        raise TypeError(f"unexpected argument {a!r}")
