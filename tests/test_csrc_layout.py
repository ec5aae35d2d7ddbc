"""CPU test of the source layout of csrc/ (the files are read as text, nothing is compiled or run): every function that one
.hip unit defines and another calls is declared in msdp_common.h and nowhere else, and the Makefile's SRCS is the set of .hip
files that exist."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "manisdp-matlab_amd", "csrc")

_HEAD = re.compile(r'^(?:extern\s+"C?"\s+)?(?:[\w:<>]+[\s*&]+)+?(msdp_\w+)\s*\(')


def _strip(txt):
    """The text without comments, string and character literals and preprocessor lines."""
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r'"(?:\\.|[^"\\\n])*"', '""', txt)
    txt = re.sub(r"'(?:\\.|[^'\\\n])'", "' '", txt)
    txt = re.sub(r"//[^\n]*", "", txt)
    txt = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", "", txt, flags=re.M)
    return txt


def _file_scope(txt):
    """(text, terminator) of every statement at file scope: terminator ';' for a declaration, '{' for what opens a body."""
    depth, start, out = 0, 0, []
    for i, c in enumerate(txt):
        if c == "{":
            if depth == 0:
                out.append((txt[start:i], "{"))
            depth += 1
        elif c == "}":
            depth -= 1
            if depth == 0:
                start = i + 1
        elif c == ";" and depth == 0:
            out.append((txt[start:i], ";"))
            start = i + 1
    return out


def _scan(path):
    """Names of the external msdp_* functions a .hip file defines, and of those it only declares."""
    defined, declared = set(), set()
    for stmt, end in _file_scope(_strip(open(path).read())):
        stmt = " ".join(stmt.split())
        if re.match(r"(?:template\s*<[^>]*>\s*)?(?:static|inline|typedef|using|struct|enum)\b", stmt) or "__global__" in stmt:
            continue
        m = _HEAD.match(stmt)
        if not m or "=" in stmt[:m.start(1)]:
            continue
        (defined if end == "{" else declared).add(m.group(1))
    return defined, declared - defined


def _units():
    return {os.path.basename(p): _scan(p) for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")))}


def test_the_scanner_tells_definitions_from_declarations(tmp_path):
    f = tmp_path / "x.hip"
    f.write_text('#define A(x) \\\n  msdp_m(x);\n// int msdp_c(int);\nint msdp_a(int x) { return msdp_b(x); }\n'
                 'static int msdp_s(int);\nint msdp_b(msdp_handle h,\n    int y = 1);   // msdp_other.hip\n'
                 'extern "C" int msdp_e(void) { return 0; }\nextern "C" int msdp_f(void);\nsize_t msdp_g();\n'
                 'const char* msdp_h(void);\nint msdp_a(int x);\n')
    defined, declared = _scan(str(f))
    assert defined == {"msdp_a", "msdp_e"}
    assert declared == {"msdp_b", "msdp_f", "msdp_g", "msdp_h"}


def test_cross_unit_functions_are_declared_in_the_common_header_only():
    units = _units()
    assert len(units) > 10
    owner = {}
    for unit, (defined, _) in units.items():
        for name in defined:
            owner.setdefault(name, unit)
    bad = sorted((unit, name, owner[name]) for unit, (_, declared) in units.items() for name in declared
                 if name in owner and owner[name] != unit)
    assert not bad, "declared by hand instead of through msdp_common.h (unit, function, defining unit): %s" % bad


def test_makefile_sources_are_the_hip_files_that_exist():
    mk = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    m = re.search(r"^SRCS\s*:?=\s*(.*)$", mk, flags=re.M)
    assert m
    srcs = re.findall(r"[\w.]+\.hip", m.group(1))
    assert len(srcs) == len(set(srcs)), "a unit is listed twice"
    present = {os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hip"))}
    assert not set(srcs) - present, "listed in SRCS but missing: %s" % sorted(set(srcs) - present)
    assert not present - set(srcs), "in csrc/ but not in SRCS: %s" % sorted(present - set(srcs))
