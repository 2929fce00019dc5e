"""The loader of this package's HIP libraries: every binding module holds one Library, built from a file name, the
environment variable that names another file, the symbol prefix, the ABI version the binding was written for, a
name -> (restype, argtypes) table of every function the library's header declares, and the module's error class."""
import ctypes
import os

E_ARG, E_DEVICE, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3, -4      # enum lbdrn_status of include/lbdrn_hip.h
# the binding modules of this package, one per library of csrc/build.py's table, in its order
BINDINGS = ("_lib", "jp2k_dec", "resid", "tiff", "tiff_write", "quality", "pyramid", "plane3")
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class NativeError(RuntimeError):
    """A failed call of a library; `status` is the lbdrn_status it returned (None for host-side failures)."""

    def __init__(self, message, status=None):
        super().__init__(message)
        self.status = status


class Library:
    missing = "{path} not built (python lbdrn-msic_amd/csrc/build.py)"
    mismatch = "{path}: ABI version {got}, this binding is for {want}"

    def __init__(self, default, env, prefix, abi, signatures, error, **messages):
        self.default, self.env, self.prefix, self.abi, self.signatures, self.error = default, env, prefix, abi, signatures, error
        self.path = os.environ.get(env) or os.path.join(_ROOT, default)
        self.__dict__.update(messages)      # missing=, mismatch=: the main library words them differently
        self.loaded = None

    def lib(self):
        if self.loaded is None:
            if not os.path.exists(self.path):
                raise self.error(self.missing.format(path=self.path))
            L = ctypes.CDLL(self.path)
            for name, (res, args) in self.signatures.items():
                fn = getattr(L, name)      # AttributeError = ABI mismatch: fail loudly
                fn.restype, fn.argtypes = res, args
            got = getattr(L, self.prefix + "abi_version")()
            if got != self.abi:
                raise self.error(self.mismatch.format(path=self.path, got=got, want=self.abi))
            self.loaded = L
        return self.loaded

    def available(self):
        try:
            self.lib()
            return True
        except (self.error, OSError):
            return False

    def last_error(self):
        return (getattr(self.lib(), self.prefix + "last_error")() or b"").decode(errors="replace")

    def check(self, rc, what):
        if rc != 0:
            raise self.error(f"{what}: {self.last_error()}", rc)
