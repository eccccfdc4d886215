"""CPU-only checks of the header reader (niwqg_amd/_abi.py) and of the binding niwqg_amd/_lib.py generates from
include/niwqg_amd.h: synthetic header text first, then the real header against the built library."""
import ctypes
import os
import re

import pytest

from niwqg_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SYNTHETIC = """
/* a comment with nq_fake(int x); and ((( unbalanced
 * parentheses ) */
#ifndef H
#define H
extern "C" {
typedef struct nq_ctx nq_ctx;
enum { NQ_ONE = 1, NQ_TWO = 2 /* nq_fake2(int y); */ };
#define NQ_ROWS 6
#define NQ_BYTES ((NQ_ROWS + 3) * NQ_TWO * 8)     // nq_fake3(int z);
typedef struct nq_params {
  int model;          /* NQ_MODEL_* */
  double nu, nu4, mu;
  int flag;
} nq_params;
typedef int (*nq_exchange_fn)(void* user, int group, int to_y);
typedef int (*nq_allreduce_fn)(void* user, int which);
int nq_broken(nq_ctx* ctx,
              const double *p,      /* ) */
              int which /* 0: q */, void * const * b);
int nq_a(void);
const char* nq_text(const nq_ctx* ctx);
long long nq_count(nq_ctx** out, const void* const* planes, unsigned long long seed);
void* nq_handle(nq_ctx* ctx, nq_exchange_fn exchange, const nq_params* p);
}
#endif
"""


def test_synthetic_header():
    prototypes, constants, fields = _abi.read(SYNTHETIC)
    assert [(n, r, [t for t, _ in p]) for n, r, p in prototypes] == [
        ("nq_broken", "int", ["nq_ctx*", "const double*", "int", "void* const*"]),
        ("nq_a", "int", []),
        ("nq_text", "const char*", ["const nq_ctx*"]),
        ("nq_count", "long long", ["nq_ctx**", "const void* const*", "unsigned long long"]),
        ("nq_handle", "void*", ["nq_ctx*", "nq_exchange_fn", "const nq_params*"])]
    assert [n for _, n in prototypes[0][2]] == ["ctx", "p", "which", "b"]
    assert constants == {"NQ_ONE": 1, "NQ_TWO": 2, "NQ_ROWS": 6, "NQ_BYTES": 144}
    assert fields == [("model", "int"), ("nu", "double"), ("nu4", "double"), ("mu", "double"), ("flag", "int")]


def test_enumerator_without_a_value_is_an_error():
    with pytest.raises(ValueError, match="NQ_B"):
        _abi.read("enum { NQ_A = 0, NQ_B };")


def test_define_that_is_not_integer_arithmetic_is_an_error():
    with pytest.raises(ValueError, match="NQ_X"):
        _abi.read("#define NQ_X (1 << 4)\n")
    with pytest.raises(ValueError, match="NQ_X"):
        _abi.read("#define NQ_X __import__('os')\n")


@pytest.fixture(scope="module")
def built():
    import niwqg_amd
    niwqg_amd.build()
    from niwqg_amd import _lib
    return _lib


def test_unknown_spelling_names_function_and_parameter():
    from niwqg_amd import _lib
    with pytest.raises(TypeError, match=r"nq_b\b.*'x'.*'short'"):
        _lib.signature(_abi.read("int nq_b(short x);")[0][0])
    with pytest.raises(TypeError, match=r"nq_c\b.*return value.*'short\*'"):
        _lib.signature(_abi.read("short* nq_c(int x);")[0][0])
    assert _lib.signature(_abi.read("void* nq_d(const int *n, nq_ctx* const* c);")[0][0]) == (
        [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p)], ctypes.c_void_p)


def _header():
    return open(os.path.join(ROOT, "include", "niwqg_amd.h")).read()


def test_every_prototype_is_typed(built):
    prototypes = _abi.read(_header())[0]
    L = built.lib()
    assert len(built.EXPORTS) == len(prototypes) and len(prototypes) >= 131
    assert all(isinstance(e, str) for e in built.EXPORTS)
    for name, ret, params in prototypes:
        fn = getattr(L, name)
        assert len(fn.argtypes) == len(params), name
        if ret != "int":
            assert fn.restype is not ctypes.c_int and fn.restype is not None, name
        else:
            assert fn.restype is ctypes.c_int, name
    assert L.nq_coeff_patch.argtypes[3] is ctypes.POINTER(ctypes.c_int)
    assert L.nq_coeff_near_contour.argtypes[4] is ctypes.POINTER(ctypes.c_int)
    assert L.nq_field_doubles.restype is ctypes.c_longlong and L.nq_stream.restype is ctypes.c_void_p
    assert L.nq_last_error.restype is ctypes.c_char_p


def test_constants_are_the_headers(built):
    text = _header()
    pairs = re.findall(r"\b(NQ_\w+) = (\d+)\b", text) + re.findall(r"^#define (NQ_\w+) (\d+)$", text, flags=re.M)
    assert len(pairs) >= 80
    for name, value in pairs:
        assert getattr(built, name[3:]) == int(value), name
    assert (built.COUPLED, built.UNCOUPLED, built.QG, built.YBJ) == (0, 1, 2, 3)
    assert built.PDF_DEVICE_BYTES == (3 * (1024 + 3) + 128 * 128 + 1) * 8 + 6 * 8192 * 8
    from niwqg_amd import _anysize, slab
    assert (slab.PH_PRODUCTS, slab.PH_BUDGET_FINISH, _anysize.EW_FILL, _anysize.RD_MAXABSRE) == (0, 7, 12, 6)


def test_params_is_the_headers_struct(built):
    fields = _abi.read(_header())[2]
    ctype = {"int": ctypes.c_int, "double": ctypes.c_double}
    assert len(fields) == 19
    assert built.Params._fields_ == [(name, ctype[t]) for name, t in fields]
    size = align = 0
    for _, t in fields:                     # the C layout rule: every member at the next multiple of its own size
        n = ctypes.sizeof(ctype[t])
        size = (size + n - 1) // n * n + n
        align = max(align, n)
    assert ctypes.sizeof(built.Params) == (size + align - 1) // align * align


def test_symbol_the_library_lacks_is_a_runtime_error(built, monkeypatch):
    extra = _abi.read(_header().replace("int nq_sync(nq_ctx* ctx);", "int nq_sync(nq_ctx* ctx);\nint nq_not_in_the_library(nq_ctx* ctx);"))[0]
    assert len(extra) == len(built.PROTOTYPES) + 1
    monkeypatch.setattr(built, "PROTOTYPES", extra)
    monkeypatch.setattr(built, "_lib", None)
    with pytest.raises(RuntimeError, match="nq_not_in_the_library"):
        built.lib()
    assert built._lib is None
