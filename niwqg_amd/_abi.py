"""Reader of the C header (include/niwqg_amd.h): what _lib.py binds is read from it, nothing is restated in Python.

Plain text in, plain Python out (no ctypes here).  It reads the C this header is written in, not C: prototypes of plain
parameters, anonymous enums whose enumerators all carry ``= n``, integer ``#define``s and the flat ``struct nq_params``.
"""
import re


def spelling(c_type):
    """one spelling per C type: single blanks, ``*`` tight to what it follows (``const double *p`` -> ``const double* p``)"""
    return re.sub(r"\*(?=\w)", "* ", re.sub(r"\s*\*\s*", "*", " ".join(c_type.split())))


def read(text):
    """(prototypes, constants, fields) of the header text:
    prototypes [(name, return spelling, [(parameter spelling, parameter name)])] of every nq_* function, in order;
    constants {"NQ_X": int} of every enumerator and every #define NQ_X of integers and earlier NQ_ names;
    fields [(name, "int" | "double")] of struct nq_params, in order."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {}
    for body in re.findall(r"\benum\s*\{([^}]*)\}", text):
        for item in filter(None, (i.strip() for i in body.split(","))):
            m = re.fullmatch(r"(NQ_\w+)\s*=\s*(-?\d+)", item)
            if not m:
                raise ValueError("enumerator %r: every enumerator states its value (NQ_X = n)" % item)
            constants[m.group(1)] = int(m.group(2))
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(NQ_\w+)[ \t]+(.+)$", text, flags=re.M):
        expr = re.sub(r"NQ_\w+", lambda m: str(constants[m.group()]), value)
        if not re.fullmatch(r"[\d\s+*()]+", expr):
            raise ValueError("#define %s %s: not an expression of integers, NQ_ names, + * ( )" % (name, value.strip()))
        constants[name] = int(eval(expr))
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    fields = []
    for body in re.findall(r"\bstruct\s+nq_params\s*\{([^}]*)\}", text):
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = re.fullmatch(r"(int|double)\s+(\w+(?:\s*,\s*\w+)*)", decl)
            if not m:
                raise ValueError("struct nq_params: %r is not a list of int or double members" % decl)
            fields += [(n.strip(), m.group(1)) for n in m.group(2).split(",")]
    prototypes = []
    for ret, name, params in re.findall(r"(?:^|(?<=[;{}]))\s*([\w\s*]+?)\s*\b(nq_\w+)\s*\(([^()]*)\)\s*;", text):
        params = [] if params.strip() == "void" else [re.fullmatch(r"(.*?)(\w*)", spelling(p)).groups() for p in params.split(",")]
        prototypes.append((name, spelling(ret), [(t.strip(), n) for t, n in params]))
    return prototypes, constants, fields
