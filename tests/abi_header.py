"""include/mrt.h read as text, and the rules that hold the Python binding
(metal-renderer_amd/mrt.py: its constants, its Structure classes and its table
of argument types) against it.  mismatches() takes the header's text, so that a
test can hand it a doctored header and see the edit reported."""
import ctypes
import re

SCALARS = {"uint8_t": ctypes.c_uint8, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
           "int64_t": ctypes.c_int64, "int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double,
           "size_t": ctypes.c_size_t}
# the block of constants at the top of mrt.py: NAME there is MRT_NAME in the header
CONSTANTS = re.compile(r"(FLAG|BVH|DISPLAY|EXCHANGE)_[A-Z_]+|COMM_ID_BYTES|REFINE_SEED_XOR|ERR_COMM")


class Header:
    """prototypes: [(name, return type, [declarator, ...])]; structs: {name:
    [declarator, ...]}; defines and status: {name: value}.  A declarator is
    (base type, pointer depth, name, [array dimensions])."""

    def __init__(self, text):
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        self.defines = {m.group(1): int(m.group(2), 0) for m in
                        re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(MRT_\w+)[ \t]+(0[xX][0-9a-fA-F]+|\d+)[uUlL]*[ \t]*$", text, re.M)}
        enum = re.search(r"typedef\s+enum\s+mrt_status\s*\{(.*?)\}\s*mrt_status\s*;", text, re.S)
        self.status = {m.group(1): int(m.group(2)) for m in re.finditer(r"(MRT_\w+)\s*=\s*(-?\d+)", enum.group(1))}
        self.structs = {}
        for m in re.finditer(r"typedef\s+struct\s+(mrt_\w+)\s*\{(.*?)\}\s*(mrt_\w+)\s*;", text, re.S):
            assert m.group(1) == m.group(3), m.group(0)
            self.structs[m.group(1)] = [d for decl in m.group(2).split(";") if decl.strip() for d in declarators(decl)]
        self.prototypes = []
        for m in re.finditer(r"^[ \t]*(int|const\s+char\s*\*)\s*(mrt_\w+)\s*\(([^)]*)\)\s*;", text, re.M):
            params = [] if m.group(3).strip() in ("", "void") else m.group(3).split(",")
            self.prototypes.append((m.group(2), " ".join(m.group(1).split()), [declarators(p)[0] for p in params]))


def declarators(decl):
    """'const float* a' or 'float right[3], up[3]' -> [(base, pointer depth, name, dims), ...]"""
    first, *rest = decl.split(",")
    head = re.match(r"\s*((?:const\s+)?\w+(?:\s+const)?)\s*(.*)$", first, re.S)
    base = head.group(1).replace("const", "").strip()
    out = []
    for d in [head.group(2)] + rest:
        m = re.match(r"\s*(\**)\s*(?:const\s+)?(\w+)?\s*((?:\[\d+\])*)\s*$", d)
        assert m, decl
        out.append((base, len(m.group(1)), m.group(2), [int(n) for n in re.findall(r"\d+", m.group(3))]))
    return out


def c_name(cls):
    """SceneDesc -> mrt_scene_desc"""
    return "mrt" + re.sub("([A-Z])", r"_\1", cls.__name__).lower()


def struct_classes(mrt):
    return {c_name(c): c for c in vars(mrt).values()
            if isinstance(c, type) and issubclass(c, ctypes.Structure) and "_fields_" in vars(c)}


def spell(t):
    if t is None:
        return "nothing"
    dims = ""
    while issubclass(t, ctypes.Array):          # in C's order: (c_float * 4) * 8 is c_float[8][4]
        dims, t = dims + f"[{t._length_}]", t._type_
    if dims:
        return spell(t) + dims
    return f"POINTER({spell(t._type_)})" if issubclass(t, ctypes._Pointer) else t.__name__


def same(a, b):
    """ctypes types, arrays by element type and length, pointers by pointee"""
    for kind in (ctypes.Array, ctypes._Pointer):
        if issubclass(a, kind) or issubclass(b, kind):
            return (issubclass(a, kind) and issubclass(b, kind) and getattr(a, "_length_", 0) == getattr(b, "_length_", 0)
                    and same(a._type_, b._type_))
    return a is b


def array_of(t, dims):
    for n in reversed(dims):
        t = t * n
    return t


def mirrors_of_field(d, classes):
    """The one ctypes type a struct member may have."""
    base, stars, _, dims = d
    if stars:
        t = ctypes.c_char_p if (base, stars) == ("char", 1) else ctypes.c_void_p
    else:
        t = SCALARS.get(base) or classes.get(base)
    return [array_of(t, dims)] if t else []


def mirrors_of_param(d, classes):
    """The ctypes types an argument may have: exactly one for a scalar, a string
    and an array; c_void_p or POINTER(the pointee's mirror) for another pointer."""
    base, stars, _, dims = d
    if dims:                                    # T name[N]: a ctypes array of T
        return [array_of(SCALARS[base], dims)] if not stars and base in SCALARS else []
    if not stars:
        return [SCALARS[base]] if base in SCALARS else []
    if (base, stars) == ("char", 1):
        return [ctypes.c_char_p]
    pointee = ctypes.c_void_p if stars > 1 else SCALARS.get(base) or classes.get(base)   # opaque handle, void: none
    return [ctypes.c_void_p] + ([ctypes.POINTER(pointee)] if pointee else [])


def mismatches(header_text, mrt):
    """Every disagreement between the header and mrt.py, one line each, naming the entry."""
    h, bad = Header(header_text), []
    classes = struct_classes(mrt)

    # names
    declared = [name for name, _, _ in h.prototypes]
    for label, names in (("the header", declared), ("EXPORTED", list(mrt.EXPORTED))):
        bad += [f"{n}: twice in {label}" for n in sorted(set(names)) if names.count(n) > 1]
    table = set(mrt._ABI)
    bad += [f"{n}: declared in the header, not in the table" for n in sorted(set(declared) - table)]
    bad += [f"{n}: in the table, not declared in the header" for n in sorted(table - set(declared))]
    bad += [f"{n}: EXPORTED and the table differ" for n in sorted(table ^ set(mrt.EXPORTED))]

    # arguments
    for name, ret, params in h.prototypes:
        if ret != "int" and name != "mrt_last_error":
            bad.append(f"{name}: returns {ret}, the binding assumes int")
        if name not in mrt._ABI:
            continue
        args = mrt._ABI[name]
        if len(args) != len(params):
            bad.append(f"{name}: {len(params)} parameters in the header, {len(args)} in the table")
            continue
        for i, (d, t) in enumerate(zip(params, args)):
            allowed = mirrors_of_param(d, classes)
            if not any(same(t, a) for a in allowed):
                bad.append(f"{name}: argument {i} ({d[2]}) is {spell(t)}, the header wants "
                           + (" or ".join(spell(a) for a in allowed) or f"a type this check does not know ({d[0]})"))

    # structs
    bad += [f"{n}: struct without a Structure class" for n in sorted(set(h.structs) - set(classes))]
    bad += [f"{n}: Structure class {classes[n].__name__} without a struct in the header" for n in sorted(set(classes) - set(h.structs))]
    for n, fields in h.structs.items():
        if n not in classes:
            continue
        mine = classes[n]._fields_
        if [d[2] for d in fields] != [k for k, _ in mine]:
            bad.append(f"{n}: fields {[d[2] for d in fields]} in the header, {[k for k, _ in mine]} in {classes[n].__name__}")
            continue
        for d, (k, t) in zip(fields, mine):
            allowed = mirrors_of_field(d, classes)
            if not any(same(t, a) for a in allowed):
                bad.append(f"{n}.{k}: is {spell(t)}, the header wants " + (" or ".join(spell(a) for a in allowed) or d[0]))

    # constants
    values = {**h.defines, **h.status}
    names = [k for k in vars(mrt) if CONSTANTS.fullmatch(k)]
    if not {"FLAG_PRECISE", "BVH_DEVICE_PLOC", "DISPLAY_RESOLVED", "EXCHANGE_OVERLAP", "COMM_ID_BYTES", "REFINE_SEED_XOR",
            "ERR_COMM"} <= set(names):
        bad.append("constants: the block at the top of mrt.py was not found")
    for k in names:
        if "MRT_" + k not in values:
            bad.append(f"{k}: no MRT_{k} in the header")
        elif values["MRT_" + k] != getattr(mrt, k):
            bad.append(f"{k}: {getattr(mrt, k)} here, MRT_{k} is {values['MRT_' + k]}")
    return bad
