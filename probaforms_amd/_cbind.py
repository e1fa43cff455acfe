"""The one ctypes loader of the package's native libraries, and the one copy of the tensor-argument validation.

A binding module holds its constants, ctypes structures and signature table and one `LIBRARY = Library(...)`; `lib` and
`check` are that object's `load` and `check`.  Nothing here needs a GPU at import.  There is NO fallback: a missing or
stale library, or a tensor off the HIP device, raises.
"""
import ctypes as C
import os
import threading

import torch

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class LibraryMissing(RuntimeError):
    """a native library has not been built, or is not the build its binding is written for"""


class Library:
    """One shared library with a C ABI `<prefix>version()`, `<prefix>status_string(int)` and the entry points of
    `signatures` (name -> (restype, argtypes)).

    path: the .so; make_dir: the directory `make -C` builds it in; abi_version: what `<prefix>version()` must report;
    missing: the binding's own LibraryMissing subclass; no_fallback: a sentence the "not found" message ends with;
    unsupported: (status code, exception class) where the binding reports that status as an exception of its own.

    load() returns the CDLL, opened and checked on first use; check(status, what) raises unless status is 0; `loaded`
    tells whether a handle is cached and forget() drops it.
    """

    def __init__(self, path, make_dir, prefix, abi_version, signatures, missing, no_fallback="", unsupported=None):
        self.path, self.make_dir, self.prefix, self.abi_version = path, make_dir, prefix, abi_version
        self.signatures, self.missing, self.no_fallback = signatures, missing, no_fallback
        self.unsupported_status, self.unsupported = unsupported or (None, None)
        # `load` and `check` run on every native call, and the binding modules bind them to module-level names, so they are
        # plain functions over this cell, not bound methods: the fast path costs what a module-level function does
        handle = None
        lock = threading.Lock()

        def load():
            """the library, loaded once; raises `missing` if it has not been built or is another build"""
            if handle is None:
                return load_locked()
            return handle

        def load_locked():
            nonlocal handle
            with lock:
                if handle is None:
                    handle = self._open()         # nothing is cached when _open raises
                return handle

        def check(status, what):
            if status != 0:
                self._fail(status, what)

        def forget():
            """drop the cached handle: the next load() opens and checks the file again"""
            nonlocal handle
            with lock:
                handle = None

        self.load, self.check, self.forget, self._peek = load, check, forget, lambda: handle

    @property
    def loaded(self):
        return self._peek() is not None

    def _open(self):
        make = "`make -C %s`" % os.path.relpath(self.make_dir, _REPO)
        if not os.path.exists(self.path):
            raise self.missing("%s not found: build it with %s (or `python -c 'import __graft_entry__ as g; g.build()'`).%s"
                               % (self.path, make, self.no_fallback and " " + self.no_fallback))
        L = C.CDLL(self.path)

        def entry(name):
            fn = getattr(L, name, None)
            if fn is None:                 # same ABI version, built before this entry point was added
                raise self.missing("%s has no %s: rebuild it (%s)" % (self.path, name, make))
            fn.restype, fn.argtypes = self.signatures[name]
            return fn

        version = self.prefix + "version"
        have = int(entry(version)())
        if have != self.abi_version:
            # an older / newer build of the same library (a stale A/B variant): struct layouts and argument lists differ
            # between versions, calling through would corrupt memory silently
            raise self.missing("%s reports %s() = %d, this binding is written for %d: rebuild it (%s)"
                               % (self.path, version, have, self.abi_version, make))
        for name in self.signatures:
            entry(name)
        return L

    def _fail(self, status, what):
        if status == self.unsupported_status:
            raise self.unsupported("%s: shape not supported" % what)
        msg = getattr(self.load(), self.prefix + "status_string")(status)
        raise RuntimeError("%s failed: %s (status %d)" % (what, msg.decode() if msg else "?", status))


def ptr(t, dtype, what, nullable=False, no_cpu=""):
    """data pointer of a contiguous tensor of `dtype` on a HIP device; None passes only where the argument is nullable"""
    if t is None:
        if nullable:
            return None
        raise RuntimeError("%s is required" % what)
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("%s must be a tensor on a HIP device (got %s)%s" % (what, getattr(t, "device", type(t)), no_cpu))
    if t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError("%s must be contiguous %s (got %s, contiguous=%s)" % (what, dtype, t.dtype, t.is_contiguous()))
    return t.data_ptr()


def f32(t, what, nullable=False):
    return ptr(t, torch.float32, what, nullable)


def stream():
    return torch.cuda.current_stream().cuda_stream
