"""CPU: the environment switches of the library are one table with one reader (lws_amd/csrc/lws_switches.h).  tests/switches_main.cpp is
that header with a main of its own, compiled with g++ and run under environments chosen here: what the reader makes of a value, the
rows of the table and their defaults (as the env_int calls of the library had them before there was a table), that nothing else in
the library reads the environment, and that INTEGRATION.md section 6, the tests and the tools name switches the table has -- a
misspelt name in a test would otherwise be ignored and the test would pass without exercising anything."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BUILD = os.path.join(HERE, "_build")

# name: (kind, default, binds) -- the defaults are those of the library's env_int("NAME", default) calls before the table; a FLAG was
# used as a truth value there, an INT as a number.  LWS_HOST_THREADS' default is computed where it is used: the table says "unset".
EXPECTED = {
    # lws_capi.hip (22)
    "LWS_TEAM_FIRST": ("FLAG", 0, "CALL"), "LWS_TEAM_FP64": ("FLAG", 0, "CALL"), "LWS_TEAM_ORDERED": ("FLAG", 0, "CALL"),
    "LWS_NO_TEAM": ("FLAG", 0, "CALL"), "LWS_NO_TEAM_Q8": ("FLAG", 0, "CALL"), "LWS_NO_SYS64": ("FLAG", 0, "CALL"),
    "LWS_ONLINE64_ONE_WAVE": ("FLAG", 0, "CALL"), "LWS_ONLINE_SERIAL_TAPS": ("FLAG", 0, "CALL"), "LWS_NOFUTURE_SERIAL_TAPS": ("FLAG", 0, "CALL"),
    "LWS_NO_SYSTOLIC": ("FLAG", 0, "CREATE"), "LWS_SYSTOLIC_NO_SHORT": ("FLAG", 0, "CREATE"), "LWS_SYSTOLIC_NO_TW": ("FLAG", 0, "CREATE"),
    "LWS_SYSTOLIC_NO_R16": ("FLAG", 0, "CREATE"),
    "LWS_HOST_MONOLITHIC": ("FLAG", 0, "CALL"), "LWS_HOST_CHUNK_BINS": ("INT", 16 << 20, "CALL"), "LWS_HOST_CHUNK_EXACT": ("FLAG", 0, "CALL"),
    "LWS_HOST_PIN_MB": ("INT", 2048, "CALL"), "LWS_HOST_HALF_FIRST": ("FLAG", 1, "CALL"), "LWS_HOST_THREADS": ("INT", "unset", "CALL"),
    "LWS_HOST_REAL": ("FLAG", 1, "CALL"), "LWS_HOST_PREFAULT": ("FLAG", 1, "CALL"), "LWS_HOST_TRACE": ("FLAG", 0, "CALL"),
    # lws_band.hip (5)
    "LWS_BAND_NO_HELPERS": ("FLAG", 0, "CALL"), "LWS_BAND_SKW": ("INT", 0, "CALL"), "LWS_BAND_NLS": ("INT", 0, "CALL"),
    "LWS_BAND_NS": ("INT", 0, "CALL"), "LWS_BAND_CHUNK": ("INT", 0, "CALL"),
    # lws_online.hip (3), lws_online64.hip (1), lws_sys64.hip (1)
    "LWS_ONLINE_TABLE_TWIDDLES": ("FLAG", 0, "CREATE"), "LWS_ONLINE_LAG_PLUS": ("INT", 0, "CALL"), "LWS_ONLINE_LAYOUT": ("INT", 0, "CALL"),
    "LWS_ONLINE64_STRESS": ("INT", 0, "CALL"), "LWS_S64_CHUNK": ("INT", 1024, "CALL"),
    # lws_team.hip (4)
    "LWS_TEAM_LANES": ("INT", 0, "CALL"), "LWS_TEAM_NO_RING": ("FLAG", 0, "CALL"), "LWS_TEAM_NCH3": ("FLAG", 0, "CALL"),
    "LWS_TEAM_DBG_POISON": ("FLAG", 0, "CALL"),
    # lws_systolic.hip (4)
    "LWS_SYSTOLIC_NWG": ("INT", 0, "CALL"), "LWS_SYSTOLIC_SPIN_LIMIT": ("INT", 1 << 21, "CALL"), "LWS_SYSTOLIC_STRESS": ("INT", 0, "CALL"),
    "LWS_SYSTOLIC_ROLEMAP": ("INT", 0, "CALL"),
}

# variables of the Python package, the mex gateway, bench.py and the tests themselves: not the library's, read where they are used
NOT_THE_LIBRARYS = {"LWS_BINDING", "LWS_HIP_LIB", "LWS_MEX_FP64", "LWS_MEX_DEVICE", "LWS_MARGINS_DIR", "LWS_REFERENCE", "LWS_USE_CYTHON"}
NOT_THE_LIBRARYS_PREFIX = "LWS_BENCH_"
# files whose quoted LWS_ names are no environment variables:
#   tools/strip_experiments.py  lists preprocessor macros of lws_systolic.hip (a one-off source clean-up)
#   this file                   LWS_FOO below is the point of its test; EXPECTED is held to the table name by name
NOT_SCANNED = {os.path.join("tools", "strip_experiments.py"), os.path.join("tests", "test_switches.py")}


@pytest.fixture(scope="module")
def driver():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "switches_main")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", os.path.join(HERE, "switches_main.cpp"), "-o", exe], check=True)

    def run(*args, **env):
        """the driver's output as {name: [fields after it]}, in an environment that has exactly `env`"""
        out = subprocess.run([exe, *args], env=env, check=True, capture_output=True, text=True).stdout
        rows = [line.split() for line in out.splitlines()]
        assert len({r[0] for r in rows}) == len(rows), "a name twice"
        return {r[0]: r[1:] for r in rows}
    return run


@pytest.fixture(scope="module")
def table(driver):
    return {name: (kind, dflt if dflt == "unset" else int(dflt), when) for name, (kind, dflt, when) in driver("--table").items()}


def snapshot(driver, **env):
    return {name: (v[0] if v[0] == "unset" else int(v[0])) for name, v in driver(**env).items()}


def test_the_table_has_the_forty_switches_with_their_defaults(table):
    assert len(table) == 40
    assert table == EXPECTED


def test_unset_and_empty_give_the_defaults(driver, table):
    defaults = {name: dflt for name, (_, dflt, _) in table.items()}
    assert snapshot(driver) == defaults
    assert snapshot(driver, **{name: "" for name in table}) == defaults


def test_a_flag_is_on_for_any_non_zero_value(driver, table):
    flags = [name for name, (kind, _, _) in table.items() if kind == "FLAG"]
    for value, want in (("1", 1), ("2", 1), ("-1", 1), ("0", 0), ("abc", 0)):
        got = snapshot(driver, **{name: value for name in flags})
        assert all(got[name] == want for name in flags), (value, got)
    assert table["LWS_HOST_REAL"][1] == 1 and snapshot(driver, LWS_HOST_REAL="0")["LWS_HOST_REAL"] == 0


def test_an_int_is_atoi(driver, table):
    ints = [name for name, (kind, _, _) in table.items() if kind == "INT"]
    assert snapshot(driver, LWS_TEAM_LANES="7")["LWS_TEAM_LANES"] == 7
    for value, want in (("7", 7), ("-3", -3), ("abc", 0), ("0", 0), ("12xyz", 12)):
        got = snapshot(driver, **{name: value for name in ints})
        assert all(got[name] == want for name in ints), (value, got)


def test_one_variable_moves_one_field_and_an_unrelated_one_none(driver, table):
    base = snapshot(driver)
    assert snapshot(driver, LWS_FOO="1", LWS_TEAM_LANE="3", XLWS_NO_TEAM="1") == base
    for name, (kind, dflt, _) in table.items():
        value = "0" if dflt == 1 else "5"
        want = dict(base, **{name: 0 if dflt == 1 else (1 if kind == "FLAG" else 5)})
        assert snapshot(driver, **{name: value}) == want, name


SOURCE = (".h", ".hip", ".cpp", ".pyx", ".pxd")


def sources(*dirs):
    for d in dirs:
        for base, _, files in os.walk(os.path.join(ROOT, d)):
            for f in sorted(files):
                if f.endswith(SOURCE) or f == "Makefile":
                    path = os.path.join(base, f)
                    with open(path, encoding="utf-8", errors="replace") as fh:
                        yield os.path.relpath(path, ROOT), fh.read()


def test_the_header_holds_the_only_reader():
    readers = [path for path, text in sources(os.path.join("lws_amd", "csrc"), "include") if "getenv(" in text]
    assert readers == [os.path.join("lws_amd", "csrc", "lws_switches.h")]
    assert [path for path, text in sources("lws_amd", "include", "tools", "matlab") if "env_int" in text] == []


def test_integration_md_lists_the_tables_rows_in_its_order(table):
    with open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8") as f:
        text = f.read()
    section = re.search(r"^## 6\. Environment switches.*?(?=^## )", text, re.S | re.M).group(0)
    rows = [[c.strip() for c in line.strip().strip("|").split("|")] for line in section.splitlines() if line.startswith("| `LWS_")]
    assert [r[0].strip("`") for r in rows] == list(table), "section 6 and LWS_SWITCHES differ in their names or their order"
    for name, kind, _, when, *_ in rows:
        assert (kind.upper(), when) == (table[name.strip("`")][0], table[name.strip("`")][2]), name
    # whatever else the section names is one of the variables that are not the library's
    for name in set(re.findall(r"LWS_[A-Z0-9_]+", section)) - set(table) - {"LWS_SWITCHES", "LWS_FORCE_GENERIC"}:   # (the macro; a plan flag)
        assert name in NOT_THE_LIBRARYS or name.startswith(NOT_THE_LIBRARYS_PREFIX), name


def test_tests_and_tools_name_only_switches_there_are(table):
    """A quoted "LWS_..." (or a keyword LWS_...="..." of a dict() / env.update()) anywhere in tests/ and tools/."""
    unknown = []
    for d in ("tests", "tools"):
        for base, dirs, files in os.walk(os.path.join(ROOT, d)):
            dirs[:] = [x for x in dirs if x not in ("_build", "__pycache__")]
            for f in sorted(files):
                path = os.path.join(base, f)
                rel = os.path.relpath(path, ROOT)
                if rel in NOT_SCANNED or not f.endswith((".py", ".sh", ".cpp", ".hip", ".h", ".m", ".md")):
                    continue
                with open(path, encoding="utf-8", errors="replace") as fh:
                    text = fh.read()
                for name in re.findall(r"""["'](LWS_[A-Z0-9_]+)["']""", text) + re.findall(r"""\b(LWS_[A-Z0-9_]+)=["']""", text):
                    if name not in table and name not in NOT_THE_LIBRARYS and not name.startswith(NOT_THE_LIBRARYS_PREFIX):
                        unknown.append((rel, name))
    assert unknown == []
