"""ctypes binding of libstin_hip.so.  The C ABI is declared in include/stin_hip.h and nowhere else: _abi.py reads the
prototypes, struct layouts and integer constants from it when this module is imported.

There is NO fallback: if the shared library is missing or a symbol is absent the
import of the HIP path fails loudly (``StinLibraryError``).  Build it with
``python -c "import __graft_entry__ as g; g.build()"`` or
``make -C surface_texture_inpainting_net_amd/csrc``.
"""
import ctypes
import os

# PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7).  It MUST
# be in the process before libstin_hip.so is dlopen'ed so that the library's NEEDED libamdhip64.so.7
# resolves to that same runtime instance; loading /opt/rocm's copy next to torch's gives a second runtime
# that sees no device (hipErrorNoDevice on the first launch).
import torch  # noqa: F401  (side effect: loads the HIP runtime torch uses)

from ._abi import StinLibraryError, read_header

_HERE = os.path.dirname(os.path.abspath(__file__))
# (STIN_LIB_PATH: an alternative build of the same library, for same-box A/B runs of compile-time switches)
LIB_PATH = os.environ.get('STIN_LIB_PATH') or os.path.join(_HERE, 'libstin_hip.so')


class StinError(RuntimeError):
    pass


# SIGNATURES: name -> (restype, argtypes); STRUCTS: typedef name -> _abi.Record (pack by field name); CONSTANTS: STIN_* #define -> int
SIGNATURES, STRUCTS, CONSTANTS = read_header()

_lib = None


def load():
    """-> the ctypes CDLL with argtypes/restype set for every declared symbol."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise StinLibraryError(
            'libstin_hip.so not found at %s - the HIP extension must be built (no CPU/eager fallback exists): '
            'run `make -C %s`' % (LIB_PATH, os.path.join(_HERE, 'csrc')))
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover
        raise StinLibraryError('cannot load %s: %s' % (LIB_PATH, e))
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            raise StinLibraryError('libstin_hip.so lacks symbol %s (stale build?)' % name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(code, what=''):
    if code != 0:
        msg = load().stin_error_string(int(code)).decode()
        raise StinError('%s failed: %s (code %d)' % (what or 'stin call', msg, code))
