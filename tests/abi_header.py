"""One reader of include/scrubvae_hip.h for the tests: the prototypes, structs, #defines and status enum of the C ABI.

A regex reader of this one header, not a C parser.  Kinds are "int", "long long", "size_t", "float", "double", "pointer" and
("void" as a return only); a pointer to one of the header's own structs has that struct's name as its kind.
tests/test_abi_contract.py holds the header against scrubvae_amd/_lib.py in full; feature tests use this module only to pin a
literal (a limit's value, an exact set of names)."""
import functools
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "scrubvae_hip.h")


@functools.lru_cache(maxsize=None)
def text():
    """the header without its comments"""
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)


def defines():
    """{name: int} for every `#define SVAE_* <integer>`"""
    return {n: int(v) for n, v in re.findall(r"^[ \t]*#define[ \t]+(SVAE_\w+)[ \t]+(-?\d+)[ \t]*$", text(), re.M)}


def status():
    """{name: int}: the members of the svae_status enum"""
    body = re.search(r"typedef\s+enum\s*\{(.*?)\}\s*svae_status\s*;", text(), re.S).group(1)
    return {n: int(v) for n, v in re.findall(r"(\w+)\s*=\s*(-?\d+)", body)}


def _split(decl):
    """"const float* x" -> ("float", True, "x"): the base type, whether a `*` stands in front of the name, the declarator"""
    words = re.sub(r"\bconst\b", " ", decl).replace("*", " * ").split()
    return " ".join(w for w in words[:-1] if w != "*"), "*" in words, words[-1]


def structs():
    """{name: [(field, kind, [array extents])]} for every `typedef struct { ... } svae_*;`; a struct member's kind is its struct"""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\{(.*?)\}\s*(svae_\w+)\s*;", text(), re.S):
        fields = out[name] = []
        for stmt in filter(None, (s.strip() for s in body.split(";"))):
            first, *more = stmt.split(",")
            base, ptr, decl = _split(first)
            for decl, ptr in [(decl, ptr)] + [(d.replace("*", "").strip(), "*" in d) for d in more]:
                extents = [int(defines().get(e, e)) for e in re.findall(r"\[(\w+)\]", decl)]
                fields.append((decl.split("[")[0], "pointer" if ptr else base, extents))
    return out


def declarations():
    """{name: (return kind, [argument kinds])} for every svae_* function prototype"""
    out, own = {}, structs()
    for ret, name, args in re.findall(r"^[ \t]*([a-z_][\w ]*?)[ \t]+(svae_\w+)[ \t]*\(([^()]*)\)\s*;", text(), re.M):
        split = [] if args.strip() == "void" else map(_split, args.split(","))
        out[name] = (" ".join(ret.split()), [(base if base in own else "pointer") if ptr else base for base, ptr, _ in split])
    return out


def declared(prefix):
    """the declared function names that start with `prefix`"""
    return {n for n in declarations() if n.startswith(prefix)}
