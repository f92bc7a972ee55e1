"""What the host tests read out of include/*.h: the entry points a header declares, the structs it typedefs, and integer
expressions (sizeof, offsetof, #define and enum values) as gcc evaluates them against it."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


def headers():
    return sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h"))


def _code(header):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, header)).read(), flags=re.S)


def declared(header):
    """the entry points include/<header> declares, sorted"""
    return sorted(set(re.findall(r"\b(segmif_[a-z0-9_]+)\s*\(", _code(header))))


def structs(header):
    """{struct name: [field names]} of the structs include/<header> typedefs, both in its order"""
    out = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", _code(header)):
        decls = [d for stmt in body.split(";") for d in stmt.split(",") if d.strip()]
        out[name] = [re.search(r"(\w+)\s*(\[[^\]]*\])?\s*$", d).group(1) for d in decls]
    return out


def c_ints(header, exprs, tmp_path):
    """[int]: each C integer expression of `exprs`, compiled against include/<header>"""
    stem = header[:-2]
    src, exe = tmp_path / (stem + "_probe.c"), tmp_path / (stem + "_probe")
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{header}"\nint main(void){{\n'
                   + "".join(f'printf("%lld\\n", (long long)({e}));\n' for e in exprs) + "return 0;}\n")
    subprocess.check_call(["gcc", "-I", INCLUDE, str(src), "-o", str(exe)])
    return [int(x) for x in subprocess.check_output([str(exe)]).split()]
