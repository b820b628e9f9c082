"""The C ABI as ctypes, read from the text of include/piccolo_hip.h: the header is the only place an entry point, a struct or a constant
is written down.  Plain `re` on the text without its comments and preprocessor lines; no compiler, no GPU.

How a declarator becomes a ctype (the header's own convention: every pointer is a DEVICE pointer unless its name ends in `_host`):
  int, int32_t, int64_t, size_t, float, double, ...   by type name (SCALARS)
  const char *                                         c_char_p
  T *const *x_host                                     POINTER(c_void_p): a host array of addresses
  scalar *x_host                                       POINTER(ctype): a host array or a host out-parameter
  const Struct *x                                      POINTER(Struct): a parameter block the library reads on the host
  every other pointer (void *, scalar *, Struct *)     c_void_p: a device address, a stream, a handle
  a field `T x[n]`                                     ctype * n
A declarator the rules do not know raises PiccoloHipError with the file and the declaration; nothing falls back to c_void_p.
To add an entry point: declare it in the header and name its host arrays `*_host`.
"""
import ctypes as C
import re

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
HOST_NAMES = {"formats"}        # host arrays the header names without the suffix; renaming them (`formats_host`) waits for the next ABI bump


class PiccoloHipError(RuntimeError):
    pass


class Header:
    """constants: NAME -> int of every `#define NAME <integer>`; structs: typedef name -> ctypes.Structure; signatures: function ->
    (restype, argtypes)."""

    def __init__(self, text, path="<header>"):
        self.path, self.constants, self.structs, self.signatures = path, {}, {}, {}
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
        for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+\(?[ \t]*(-?\d+)[ \t]*\)?[ \t]*$", text, flags=re.M):
            self.constants[name] = int(value)
        text = re.sub(r'^[ \t]*#[^\n]*|extern\s+"C"\s*\{', "", text, flags=re.M)
        text = re.sub(r"typedef\s+struct\s*\w*\s*\{(.*?)\}\s*(\w+)\s*;", self._struct, text, flags=re.S)
        for decl in (" ".join(d.split()) for d in text.split(";")):
            if decl in ("", "}"):                # (the brace closes extern "C")
                continue
            m = re.fullmatch(r"(.*?)(\w+) ?\((.*)\)", decl)
            if not m:
                raise PiccoloHipError("%s: not a prototype: %r" % (path, decl))
            params = [] if m[3].strip() == "void" else m[3].split(",")
            self.signatures[m[2]] = (self._ctype(m[1], decl, ret=True)[1], [self._ctype(p, decl)[1] for p in params])

    @classmethod
    def read(cls, path):
        try:
            with open(path) as f:
                return cls(f.read(), path)
        except OSError as e:
            raise PiccoloHipError("%s: cannot read the C header the binding is derived from (%s)" % (path, e)) from None

    def constant(self, name):
        if name not in self.constants:
            raise PiccoloHipError("%s: no `#define %s <integer>`" % (self.path, name))
        return self.constants[name]

    def _struct(self, m):
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in m[1].split(";"))):
            first, *more = decl.split(",")                  # `float a, b[3]`: the later declarators share the first one's type words
            fields += [self._ctype(d, "%s: %s" % (m[2], decl)) for d in [first] + [self._split(first)[0] + d for d in more]]
        self.structs[m[2]] = type(m[2], (C.Structure,), {"_fields_": fields})
        return ""

    @staticmethod
    def _split(decl):
        m = re.fullmatch(r"\s*(.*?)(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*", decl)
        return m.groups() if m else ("", "", None)

    def _ctype(self, decl, where, ret=False):
        """-> (name, ctype) of one parameter or field declarator, or of a return type (ret: no name; `void` is None)."""
        words, name, dim = self._split(decl + (" _" if ret else ""))
        base = " ".join(w for w in words.replace("*", " ").split() if w != "const")
        stars, host = words.count("*"), name.endswith("_host") or name in HOST_NAMES
        const = "const" in words.split("*")[0].split()
        if stars == 0 and (base in SCALARS or ret and base == "void"):
            t = SCALARS.get(base)
        elif stars == 1 and base == "char" and const:
            t = C.c_char_p
        elif stars == 1 and base in self.structs:
            t = C.POINTER(self.structs[base]) if const or host else C.c_void_p
        elif stars == 1 and (base in SCALARS or base == "void"):
            t = C.POINTER(SCALARS[base]) if host and base != "void" else C.c_void_p
        elif stars == 2 and host and (base in SCALARS or base == "void"):
            t = C.POINTER(C.c_void_p)
        else:
            raise PiccoloHipError("%s: no ctypes rule for %r in %r" % (self.path, decl.strip(), where))
        return name, t * int(dim) if dim else t
