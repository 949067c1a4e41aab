"""The binding contract between include/leftrefill_hip.h and its ctypes mirror leftrefill_amd/_lib.py (tests/test_abi_cpu.py): the header
parsed once, gcc's struct layouts from one probe, and the checks.  A check returns the mismatches it found ([] = agreement), so a
doctored table can be shown to fail without touching the real one.  CPU only, no built library.  No tests here."""
import ctypes
import functools
import os
import re
import subprocess
import tempfile
from collections import namedtuple

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
Proto = namedtuple("Proto", "ret params")       # params: whitespace-normalised declarations, [] for (void)
Header = namedtuple("Header", "text protos dev_protos structs")     # text: the raw file; structs: name -> field names in order


def _protos(src):
    return {name: Proto(ret, [re.sub(r"\s+", " ", p).strip() for p in params.split(",") if p.strip() != "void"])
            for ret, name, params in re.findall(r"^(int|int64_t) (lr_\w+)\(([^;{]*)\);", src, flags=re.M)}


@functools.lru_cache(maxsize=None)
def header():
    with open(os.path.join(INCLUDE, "leftrefill_hip.h")) as f:
        text = f.read()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    dev = re.search(r"^#ifdef LR_DEV_VARIANTS\b(.*?)^#endif", src, flags=re.S | re.M)      # developer builds only
    structs = {m.group(1): [re.search(r"(\w+)\s*(?:\[[^\]]*\])?$", d.strip()).group(1) for decl in m.group(2).split(";") if decl.strip()
                            for d in decl.split(",")]
               for m in re.finditer(r"^typedef struct (lr_\w+) \{(.*?)\} \1;", src, flags=re.S | re.M)}
    return Header(text, _protos(src[:dev.start()] + src[dev.end():]), _protos(dev.group(1)), structs)


def c_params(name):      # the parameter declarations of entry point `name` as the header writes them, whitespace-normalised
    return {**header().protos, **header().dev_protos}[name].params


def define(name):      # the integer value of `#define name <integer>` in the header
    return int(re.search(rf"^#define {name} (-?\d+)\b", header().text, flags=re.M).group(1))


@functools.lru_cache(maxsize=None)
def c_layout():
    """{struct: {None: sizeof, field: (offsetof, sizeof)}} as gcc lays out every struct of the header: one generated probe, compiled once."""
    lines = [f'printf("{s} - %zu 0\\n", sizeof({s}));' for s in header().structs]
    lines += [f'printf("{s} {f} %zu %zu\\n", offsetof({s}, {f}), sizeof((({s}*)0)->{f}));' for s, fields in header().structs.items() for f in fields]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "leftrefill_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\nreturn 0;\n}\n"
    with tempfile.TemporaryDirectory() as d:
        subprocess.run(["gcc", "-I", INCLUDE, "-x", "c", "-", "-o", os.path.join(d, "probe")], input=prog, text=True, check=True)
        out = subprocess.run([os.path.join(d, "probe")], check=True, capture_output=True, text=True).stdout
    layout = {s: {} for s in header().structs}
    for s, f, a, b in (line.split() for line in out.splitlines()):
        layout[s][None if f == "-" else f] = int(a) if f == "-" else (int(a), int(b))
    return layout


_SCALARS = {"int": (ctypes.c_int, ctypes.c_int32), "int32_t": (ctypes.c_int, ctypes.c_int32), "int64_t": (ctypes.c_int64,), "float": (ctypes.c_float,)}


def _param_mismatch(decl, argtype, structs):
    """None if ctypes `argtype` may stand for the header parameter `decl`, else what is wrong."""
    if "*" in decl or decl.startswith("lr_stream_t "):
        if argtype in (ctypes.c_void_p, ctypes.c_char_p):
            return None
        if not (isinstance(argtype, type) and issubclass(argtype, ctypes._Pointer)):
            return f"pointer `{decl}` bound as {argtype}"
        pointee, target = re.sub(r"\bconst\b", "", decl.split("*")[0]).strip(), argtype._type_
        want = (structs.get(pointee),) if issubclass(target, ctypes.Structure) else _SCALARS.get(pointee, ())
        return None if target in want else f"`{decl}` bound as POINTER({target.__name__})"
    m = re.fullmatch(r"(?:const )?(\w+) \w+", decl)
    if not m or m.group(1) not in _SCALARS:
        return f"`{decl}`: a kind of parameter the contract does not know"
    return None if argtype in _SCALARS[m.group(1)] else f"`{decl}` bound as {argtype.__name__}"


def check_signatures(signatures, int64_returns, structs):
    """Every bound entry point (product and developer), parameter by parameter, and the int64_t returns."""
    protos, bad = {**header().protos, **header().dev_protos}, []
    for name, argtypes in signatures.items():
        if name not in protos or len(protos[name].params) != len(argtypes):
            bad.append(f"{name}: " + ("not declared" if name not in protos else f"{len(protos[name].params)} parameters, {len(argtypes)} argtypes"))
            continue
        bad += [f"{name} #{i}: {why}" for i, (decl, a) in enumerate(zip(protos[name].params, argtypes)) for why in [_param_mismatch(decl, a, structs)] if why]
    wide = {n for n, p in protos.items() if p.ret == "int64_t"}
    return bad + ([f"int64_t returns: header and INT64_RETURNS differ in {sorted(wide ^ set(int64_returns))}"] if wide != set(int64_returns) else [])


def check_twins(bf16_twins, twin):
    protos, twins = header().protos, {twin(n) for n in bf16_twins}
    declared = {n for n in protos if n.endswith("_bf16")}
    bad = [f"BF16_TWINS and the header's *_bf16 names differ in {sorted(twins ^ declared)}"] if twins != declared else []
    return bad + [f"{twin(n)}: parameters differ from {n}'s" for n in bf16_twins
                  if n in protos and twin(n) in protos and protos[n].params != protos[twin(n)].params]


def check_structs(structs):
    """Field names in order, sizeof, and every field's offset and size against the C compiler."""
    fields, layout = header().structs, c_layout()
    bad = [f"structs: header and STRUCTS differ in {sorted(set(fields) ^ set(structs))}"] if set(fields) != set(structs) else []
    for s, cls in ((s, structs[s]) for s in sorted(set(fields) & set(structs))):
        got = {None: ctypes.sizeof(cls), **{f: (getattr(cls, f).offset, getattr(cls, f).size) for f, _ in cls._fields_}}
        if list(got)[1:] != fields[s]:
            bad.append(f"{s}: fields {list(got)[1:]} != {fields[s]}")
        bad += [f"{s}.{f or 'sizeof'}: {got[f]} != {want}" for f, want in layout[s].items() if f in got and got[f] != want]
    return bad
