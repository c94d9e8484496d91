"""csrc/hipk_switch.h holds the one table of the C library's environment switches and the only calls of getenv; DESIGN.md lists
the same rows.  These checks keep the table, the call sites, the document and the names that tests and tools set in step."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pytorch-sparse-linalg-torch-amgx.cg.bicg.gmres_amd", "csrc")
HEADER = os.path.join(CSRC, "hipk_switch.h")
KINDS = {"HIPK_SW_PRESENT": "present", "HIPK_SW_OFF_IF_0": "off_if_0", "HIPK_SW_FORCE01": "force01", "HIPK_SW_INT": "int", "HIPK_SW_WORD": "word"}
ROW = re.compile(r'^\s*\{"(HIPK_[A-Z0-9_]+)", (HIPK_SW_[A-Z0-9_]+), "([^"]*)", "([^"]*)", "([^"]*)", "([^"]*)"\},\s*$', re.M)
ACCESSOR = re.compile(r'\bhipk_sw_(present|enabled|force|int|word_is)\(\s*("?)([^",)]*)\2')


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))


def _rows():
    rows = ROW.findall(_read(HEADER))
    assert len(rows) >= 40, "the switch table of hipk_switch.h was not recognised (one row per line)"
    return rows


def _design_section():
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    m = re.search(r"^## [^\n]*Environment switches[^\n]*\n(.*?)(?=^## )", text, re.M | re.S)
    assert m, "DESIGN.md has no section 'Environment switches'"
    c_part, sep, py_part = m.group(1).partition("### Python-side switches")
    assert sep, "the section has no block 'Python-side switches'"
    first_cell = re.compile(r"^\| `(HIPK_[A-Z0-9_]+)` \|", re.M)
    return first_cell.findall(c_part), first_cell.findall(py_part)


def test_getenv_only_in_the_switch_header():
    for path in _sources():
        if path != HEADER:
            assert "getenv" not in _read(path), f"{os.path.relpath(path, ROOT)} calls getenv: read the switch through csrc/hipk_switch.h"
    assert "getenv" in _read(HEADER)


def test_rows_are_unique_and_of_a_known_kind():
    rows = _rows()
    names = [r[0] for r in rows]
    assert len(set(names)) == len(names), sorted(n for n in names if names.count(n) > 1)
    for name, kind, dflt, read, meaning, used_by in rows:
        assert kind in KINDS, (name, kind)
        assert dflt and read and meaning, f"{name}: default, read-when and meaning are all stated"
        assert set(re.split(r", ", used_by)) <= {"test", "tools A/B", "user"}, (name, used_by)


def test_every_row_is_used_and_every_accessor_names_a_row():
    names = {r[0] for r in _rows()}
    used = set()
    for path in _sources():
        text = _read(path)
        if path == HEADER:
            text = text[text.index("constexpr bool hipk_sw_streq"):]   # (below the table: the accessors' definitions)
        for m in ACCESSOR.finditer(text):
            if path == HEADER and m.group(2) == "":
                continue   # the macro definitions themselves: hipk_sw_present(name) ...
            assert m.group(2) == '"', f"{os.path.relpath(path, ROOT)}: {m.group(0)}...: the switch is named by a string literal"
            assert m.group(3) in names, f"{os.path.relpath(path, ROOT)}: {m.group(3)} is not a row of hipk_switches"
            used.add(m.group(3))
    assert names - used == set(), f"rows that no code reads: {sorted(names - used)}"


def test_names_put_into_the_environment_are_rows():
    """A quoted "HIPK_..." (or "HIPK_...=value") in tests/, bench.py and tools/*.py names a switch, unless include/hipk.h declares
    the name: ABI constants such as HIPK_F64 and HIPK_ERR_* are never put into an environment."""
    abi = set(re.findall(r"\b(HIPK_[A-Z0-9_]+) = -?\d", _read(os.path.join(ROOT, "include", "hipk.h"))))   # enumerators
    assert "HIPK_F64" in abi and "HIPK_ERR_ARG" in abi
    c_names = {r[0] for r in _rows()}
    assert not abi & c_names
    py_names = set(_design_section()[1])
    files = glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")) + [os.path.join(ROOT, "bench.py")]
    me = os.path.abspath(__file__)
    unknown = {}
    for path in files:
        if os.path.abspath(path) == me:
            continue
        for name in re.findall(r"""["'](HIPK_[A-Z0-9_]+)(?:=[^"']*)?["']""", _read(path)):
            if name not in c_names and name not in py_names and name not in abi:
                unknown.setdefault(name, []).append(os.path.relpath(path, ROOT))
    assert not unknown, f"switches that are neither a row of hipk_switches nor of DESIGN.md's Python block: {unknown}"


def test_used_by_says_test_exactly_when_a_test_names_the_switch():
    """A row's used_by contains `test` exactly when a file under tests/ (other than this one) names the switch in quotes."""
    me = os.path.abspath(__file__)
    named = set()
    for path in glob.glob(os.path.join(ROOT, "tests", "*.py")):
        if os.path.abspath(path) != me:
            named |= set(re.findall(r"""["'](HIPK_[A-Z0-9_]+)(?:=[^"']*)?["']""", _read(path)))
    for name, _kind, _dflt, _read_when, _meaning, used_by in _rows():
        says = "test" in re.split(r", ", used_by)
        assert says == (name in named), f"{name}: used_by is '{used_by}', {'a' if name in named else 'no'} file under tests/ names it"


def test_design_lists_exactly_the_table():
    rows = _rows()
    c_doc, py_doc = _design_section()
    assert sorted(c_doc) == sorted(r[0] for r in rows), sorted(set(c_doc) ^ {r[0] for r in rows})
    assert not set(py_doc) & set(c_doc)
    # kind and default as the header states them
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    for name, kind, dflt, _read_when, _meaning, _used in rows:
        m = re.search(r"^\| `%s` \| ([a-z0-9_]+) \| ([^|]*) \|" % name, text, re.M)
        assert m and m.group(1) == KINDS[kind] and m.group(2).strip() == dflt, (name, m and m.groups())
        # ... and who uses it (the last cell)
        m = re.search(r"^\| `%s` \|.*\| ([^|]*) \|$" % name, text, re.M)
        assert m and m.group(1).strip() == _used, (name, m and m.group(1), _used)
