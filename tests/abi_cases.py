"""What the host tests ask of the C ABI, stated once: the test side's own reading of include/xmca_hip.h (regular expressions over the
comment-free text), the check every test of a new entry point makes (`check_entry`), and the comparison of one row of the binding
table `_hip.SIGNATURES` with its declaration, type by type (`check_types`)."""
import ctypes
import functools
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "xmca_hip.h")

# C spelling -> what the binding must say.  A pointer may be bound as c_void_p, or typed when the type is the pointee's.
VALUE_TYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "uint64_t": ctypes.c_uint64,
               "uint32_t": ctypes.c_uint32}
RETURN_TYPES = {"int": ctypes.c_int, "void": None, "const char*": ctypes.c_char_p, "long long": ctypes.c_longlong}
POINTEES = {"void": (), "xmca_handle": (), "xmca_comm": (),                       # pointee of `[const] pointee*` -> typed forms allowed
            "xmca_handle*": (ctypes.POINTER(ctypes.c_void_p),), "xmca_comm*": (ctypes.POINTER(ctypes.c_void_p),),
            "double": (ctypes.POINTER(ctypes.c_double),), "int": (ctypes.POINTER(ctypes.c_int),),
            "int64_t": (ctypes.POINTER(ctypes.c_int64),), "char": (ctypes.c_char_p,), "unsigned char": (ctypes.c_char_p,)}


def header_text(comments=False):
    """include/xmca_hip.h as it is, or (the default) without its comments."""
    text = open(HEADER).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


@functools.lru_cache(maxsize=None)
def header_declarations():
    """name -> (return type, (arguments as the header spells them, e.g. "xmca_handle* h", ...)) of every entry point; () for (void)."""
    code = re.sub(r"^[ \t]*#.*$", "", header_text(), flags=re.M)
    out = {}
    for ret, name, args in re.findall(r"^([\w \t*]+?)\b(xmca_\w+)\s*\(([^;]*)\)\s*;", code, flags=re.M):
        args = tuple(" ".join(a.split()) for a in args.split(","))
        out[name] = (c_type(ret), () if args == ("void",) else args)
    return out


def c_type(spelling, named=False):
    """A C type as a key of the tables above: one space between words, none around a `*`; named: without the argument's name."""
    if named:
        spelling = re.sub(r"(?<=[\s*])\w+$", "", spelling.strip())
    return re.sub(r"\s*\*\s*", "*", " ".join(spelling.split()))


def header_arguments(name):
    assert name in header_declarations(), "%s is not declared in include/xmca_hip.h" % name
    return list(header_declarations()[name][1])


def header_define(name):
    """The integer the header gives `#define name`."""
    d = re.search(r"#define\s+%s\s+\(?(-?\d+)\)?" % name, header_text())
    assert d, "%s is not defined in include/xmca_hip.h" % name
    return int(d.group(1))


def header_abi_version():
    return header_define("XMCA_ABI_VERSION")


def check_entry(name, n_args=None):
    """`name` is declared in the header with `n_args` arguments (None: however many it declares), exported by the library, and bound
    with that many argument types and an int result."""
    from xmca_amd import _hip
    args = header_arguments(name)
    if n_args is not None:
        assert len(args) == n_args, (name, args)
    lib = _hip.load_library()
    assert hasattr(lib, name), "%s is not exported" % name
    assert name in _hip.SIGNATURES, "%s is not bound" % name
    restype, argtypes = _hip.SIGNATURES[name]
    assert restype is ctypes.c_int and len(argtypes) == len(args), (name, args, argtypes)
    assert getattr(lib, name).argtypes == list(argtypes), name


def check_types(name, restype, argtypes):
    """(restype, argtypes) - a row of the binding table - says what the header declares for `name`: the return type, the number of
    arguments, the exact type at every value position and a pointer of the right kind at every pointer position."""
    ret, args = header_declarations()[name]
    assert ret in RETURN_TYPES, "%s returns `%s`: the tests do not know that type" % (name, ret)
    assert restype is RETURN_TYPES[ret], (name, ret, restype)
    assert len(argtypes) == len(args), (name, args, argtypes)
    for i, (arg, bound) in enumerate(zip(args, argtypes)):
        t = c_type(arg, named=True)
        if t in VALUE_TYPES:
            assert bound is VALUE_TYPES[t], "%s, argument %d (`%s`) is bound as %s" % (name, i, arg, bound)
        else:
            pointee = re.fullmatch(r"(?:const )?(.+)\*", t)
            assert pointee and pointee.group(1) in POINTEES, "%s, argument %d (`%s`): the tests do not know that type" % (name, i, arg)
            assert bound is ctypes.c_void_p or bound in POINTEES[pointee.group(1)], "%s, argument %d (`%s`) is bound as %s" % (name, i, arg, bound)
