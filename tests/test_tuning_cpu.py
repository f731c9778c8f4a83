"""The PTMI_* tuning knobs without a GPU: csrc/ptmi_tuning.h (the struct and the parsing that ptmi.hip uses) compiled into a small host program that prints the
parsed struct.  Every knob: unset gives the documented default, values inside its domain are taken as written, everything else — below, above, far beyond
int, empty, not a number — lands inside the domain.  The domain is where the kernels are defined: PTMI_REFILL above 64 would keep a k_bvh wave in its inner
loop for ever (`while (working >= 64 - refill + 1)` with no lane working), which is why this is tested here and never on a device.

Also here, because they read source text only: the guard that keeps test_tuning_invariance_gpu.py's instance table in step with the dispatcher of ptmi.hip,
and the check that README.md's table, this file and the GPU file speak of the same variables."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "webgpu-path-tracer_amd", "csrc")
INT_MAX = 2**31 - 1

# variable, field of struct Tuning, default, lowest, highest value of the domain.  (README.md's table and the comments of ptmi_tuning.h say the same.)
INT_KNOBS = [
    ("PTMI_LDS_STACK", "lds_stack", 10, 1, 64),
    ("PTMI_WAVES_PER_CU", "waves_per_cu", 0, 0, 32),
    ("PTMI_BVH_TEAMS", "bvh_teams", 16, 1, 64),
    ("PTMI_REFILL", "refill", 32, 1, 64),
    ("PTMI_LEAF_BATCH", "leaf_batch", 16, 1, 65),
    ("PTMI_BVH_RANGE", "bvh_range", 512, 64, 65536),  # (and a multiple of 64: rounded down)
    ("PTMI_TAIL_WAVES_PER_CU", "tail_waves_per_cu", 0, 0, 32),
    ("PTMI_TAIL_PARK", "tail_park", 16, 0, 63),
    ("PTMI_BVH_CARRY", "bvh_carry", 32, 0, INT_MAX),
    ("PTMI_BVH_CARRY_SLOTS", "bvh_carry_slots", 1 << 18, 64, 1 << 22),
    ("PTMI_BVH_CARRY_LAST", "bvh_carry_last", 0, 0, INT_MAX),
    ("PTMI_BVH_CARRY_MIN_PATHS", "bvh_carry_min_paths", 4 << 20, 0, INT_MAX),
    ("PTMI_BVH_CARRY_MIN_DEPTH", "bvh_carry_min_depth", 12, 0, INT_MAX),
    ("PTMI_SORT", "sort", -1, -1, 1),
    ("PTMI_SHADE_BLOCKS_PER_CU", "shade_blocks_per_cu", 0, 0, 8),
    ("PTMI_SHADE_CONT", "shade_cont", 16, 0, 64),
    ("PTMI_TAIL_LIMIT", "tail_limit", -1, -1, INT_MAX),
    ("PTMI_PATH_BUDGET_LOG2", "path_budget_log2", 30, 16, 31),
    ("PTMI_PLACEMENT_TRIES", "placement_tries", 6, 1, 16),
]
# variable, field, default: "0" (or any number that is zero) = off, any other number = on
BOOL_KNOBS = [("PTMI_NOABORT", "noabort", 1), ("PTMI_TAIL6", "tail6", 1), ("PTMI_RENDER_AHEAD", "render_ahead", 1)]
FLAG_KNOBS = [("PTMI_DEBUG_PLACEMENT", "debug_placement")]  # set to anything = on
# the rest of README.md's table: not part of struct Tuning — read elsewhere, as text or by other programs
NOT_TUNING = {
    "PTMI_MULTI_REDUCE": "ptmi_create_multi: a word (tests/test_multi_device_gpu.py)",
    "PTMI_RCCL_LIB": "a path",
    "PTMI_BUILD_THREADS": "ptmi_host.cpp: host threads, clamped to 1..32 where it is read",
    "PTMI_LIB": "the bindings: a path",
    "PTMI_TEST_ALLOC_LIMIT": "the test-hooks build only",
    "PTMI_TEST_RCCL_FAIL": "the test-hooks build only",
    "PTMI_TEST_DENOISE_SCRATCH": "the test-hooks build only: the cap of the denoisers' scratch in bytes (tests/test_stack_geometry_gpu.py)",
    "PTMI_BENCH_SIMULATE": "bench.py only",
}
FIELDS = [k[1] for k in INT_KNOBS + BOOL_KNOBS + FLAG_KNOBS]
ALL_NAMES = [k[0] for k in INT_KNOBS + BOOL_KNOBS + FLAG_KNOBS]

DRIVER = "#include <cstdio>\n#include \"ptmi_tuning.h\"\nint main() {\n  const ptmi::Tuning t = ptmi::load_tuning_env();\n" + "".join(
    '  printf("%s=%%d\\n", (int)t.%s);\n' % (f, f) for f in FIELDS) + "  return 0;\n}\n"


def in_domain(name, v):
    """What the library makes of an in-domain value: itself (PTMI_BVH_RANGE: rounded down to a multiple of 64)."""
    return v & ~63 if name == "PTMI_BVH_RANGE" else v


@pytest.fixture(scope="module")
def parse(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ is needed to compile csrc/ptmi_tuning.h"
    d = tmp_path_factory.mktemp("tuning")
    src, exe = os.path.join(str(d), "dump_tuning.cpp"), os.path.join(str(d), "dump_tuning")
    with open(src, "w") as f:
        f.write(DRIVER)
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC, "-o", exe, src], check=True)

    def run(env):
        e = {k: v for k, v in os.environ.items() if not k.startswith("PTMI_")}
        e.update(env)
        out = subprocess.run([exe], env=e, check=True, stdout=subprocess.PIPE, text=True).stdout
        got = dict(line.split("=") for line in out.split())
        assert sorted(got) == sorted(FIELDS)
        return {k: int(v) for k, v in got.items()}

    return run


def test_the_struct_has_no_field_this_file_does_not_know():
    text = open(os.path.join(CSRC, "ptmi_tuning.h")).read()
    body = text[text.index("struct Tuning {"):text.index("};", text.index("struct Tuning {"))]
    body = re.sub(r"//[^\n]*", "", body)
    fields = re.findall(r"\b([a-z_0-9]+)\s*=\s*[^,;]+[,;]", body)
    assert sorted(fields) == sorted(FIELDS)
    assert sorted(set(re.findall(r'"(PTMI_[A-Z0-9_]+)"', text))) == sorted(ALL_NAMES)


def test_unset_gives_the_documented_defaults(parse):
    got = parse({})
    for name, field, dflt, lo, hi in INT_KNOBS:
        assert got[field] == dflt and lo <= dflt <= hi, (name, got[field])
    for name, field, dflt in BOOL_KNOBS:
        assert got[field] == dflt, name
    for name, field in FLAG_KNOBS:
        assert got[field] == 0, name


@pytest.mark.parametrize("pick", ["lowest", "highest", "inside"])
def test_values_inside_the_domain_are_taken_as_written(parse, pick):
    def value(name, lo, hi):
        if pick == "inside":
            return {"PTMI_BVH_RANGE": 4096, "PTMI_SORT": 0}.get(name, lo + (min(hi, 1 << 20) - lo) // 3 + 1)
        return lo if pick == "lowest" else hi

    env = {name: str(value(name, lo, hi)) for name, _, _, lo, hi in INT_KNOBS}
    got = parse(env)
    for name, field, _, lo, hi in INT_KNOBS:
        v = value(name, lo, hi)
        assert lo <= v <= hi
        assert got[field] == in_domain(name, v), (name, v, got[field])


def test_odd_spellings_of_a_number(parse):
    got = parse({"PTMI_REFILL": " 17", "PTMI_LEAF_BATCH": "+9", "PTMI_BVH_TEAMS": "12 teams", "PTMI_LDS_STACK": "7.9", "PTMI_BVH_RANGE": "1000", "PTMI_TAIL_PARK": "0x20"})
    assert (got["refill"], got["leaf_batch"], got["bvh_teams"], got["lds_stack"], got["bvh_range"], got["tail_park"]) == (17, 9, 12, 7, 960, 0)


OUTSIDE = ["one below", "one above", "-1000000", "1000000000", "-99999999999999999999", "99999999999999999999", "", "abc", "-", "--5"]


@pytest.mark.parametrize("how", OUTSIDE)
def test_everything_else_lands_inside_the_domain(parse, how):
    def text(lo, hi):
        return str(lo - 1) if how == "one below" else str(hi + 1) if how == "one above" else how

    got = parse({name: text(lo, hi) for name, _, _, lo, hi in INT_KNOBS})
    for name, field, dflt, lo, hi in INT_KNOBS:
        v = got[field]
        assert lo <= v <= hi, (name, text(lo, hi), v)
        if name == "PTMI_BVH_RANGE":
            assert v % 64 == 0
        # ... and at the end one would expect: the nearer one for a number, the default for what is no number
        if how in ("", "abc", "-", "--5"):
            want = dflt
        else:
            want = in_domain(name, max(lo, min(hi, int(text(lo, hi)))))
        assert v == want, (name, text(lo, hi), v, want)


@pytest.mark.parametrize("value,want", [("65", 64), ("1000", 64), ("64", 64), ("63", 63), ("1", 1), ("0", 1), ("-3", 1), ("2147483648", 64), ("", 32), ("many", 32)])
def test_refill_never_leaves_1_to_64(parse, value, want):
    """k_bvh's inner loop ends only if 64 - refill + 1 >= 1 (csrc/ptmi_kernels.h, bvh2_body: min_working)."""
    got = parse({"PTMI_REFILL": value})["refill"]
    assert got == want and 64 - got + 1 >= 1


def test_switches(parse):
    for name, field, dflt in BOOL_KNOBS:
        for text, want in (("0", 0), ("1", 1), ("2", 1), ("-1", 1), ("00", 0), ("", dflt), ("off", dflt)):
            assert parse({name: text})[field] == want, (name, text)
    for name, field in FLAG_KNOBS:
        assert parse({name: "1"})[field] == 1 and parse({name: ""})[field] == 1


# ---- README.md, this file and the GPU file name the same variables -----------------------------------------------------------------------------------------

def _readme_table():
    rows = [l for l in open(os.path.join(ROOT, "README.md")).read().splitlines() if l.startswith("| `PTMI_")]
    assert len(rows) >= 10
    return rows


def test_every_row_of_the_readme_table_is_covered_here():
    named = set()
    for row in _readme_table():
        named.update(re.findall(r"`(PTMI_[A-Z0-9_]+)`", row.split("|")[1]))
    assert named == set(ALL_NAMES) | set(NOT_TUNING), (sorted(named - set(ALL_NAMES) - set(NOT_TUNING)), sorted((set(ALL_NAMES) | set(NOT_TUNING)) - named))


def test_the_readme_states_each_domain():
    for row in _readme_table():
        cells = [c.strip() for c in row.split("|")[1:-1]]
        names = re.findall(r"`(PTMI_[A-Z0-9_]+)`", cells[0])
        if not any(n in dict((k[0], k) for k in INT_KNOBS) for n in names):
            continue
        assert len(cells) == 4, row  # variable, default, domain, meaning
        domains = [d.strip() for d in cells[2].split(",")]
        assert len(domains) == len(names), (names, domains)
        for n, d in zip(names, domains):
            k = [k for k in INT_KNOBS if k[0] == n]
            if not k:
                continue
            lo, hi = k[0][3], k[0][4]
            m = re.fullmatch(r"(-?\d+) … (\d+|2\^\d+|INT_MAX)", d.replace("2³¹−1", "INT_MAX"))
            assert m, (n, d)
            top = INT_MAX if m.group(2) == "INT_MAX" else 2 ** int(m.group(2)[2:]) if m.group(2).startswith("2^") else int(m.group(2))
            assert (int(m.group(1)), top) == (lo, hi), (n, d)


def test_every_variable_the_library_reads_is_in_the_readme_table():
    read = set()
    for f in os.listdir(CSRC):
        read.update(re.findall(r'"(PTMI_[A-Z0-9_]+)"', open(os.path.join(CSRC, f)).read()))
    assert read <= set(ALL_NAMES) | set(NOT_TUNING), sorted(read - set(ALL_NAMES) - set(NOT_TUNING))


# variables that reach a kernel argument, a grid size or the choice of a kernel instance: the GPU file sets each to at least two non-default values
REACH_KERNELS = [n for n in ALL_NAMES if n not in ("PTMI_RENDER_AHEAD", "PTMI_PLACEMENT_TRIES", "PTMI_DEBUG_PLACEMENT", "PTMI_BVH_CARRY_MIN_PATHS", "PTMI_BVH_CARRY_MIN_DEPTH")]
# (PTMI_RENDER_AHEAD, PTMI_PLACEMENT_TRIES: host scheduling, tests/test_parity_gpu.py; the two _MIN_ thresholds only decide WHETHER rays are carried:
#  the GPU file sets them to 0 wherever it forces carrying, which is their one non-default use.  PTMI_NOABORT and PTMI_TAIL6 are switches: one non-default value.)
SWITCHES = ("PTMI_NOABORT", "PTMI_TAIL6")


def test_the_gpu_file_sets_every_kernel_knob_to_two_non_default_values():
    import test_tuning_invariance_gpu as T

    defaults = {k[0]: str(k[2]) for k in INT_KNOBS + BOOL_KNOBS}
    seen = {}
    for env in T.all_environments():
        for k, v in env.items():
            assert k in ALL_NAMES, k
            if str(v) != defaults[k]:
                seen.setdefault(k, set()).add(str(v))
    for name in REACH_KERNELS:
        assert len(seen.get(name, ())) >= (1 if name in SWITCHES else 2), (name, seen.get(name))
    # nothing in it is a value the clamping would change
    dom = {k[0]: (k[3], k[4]) for k in INT_KNOBS}
    for env in T.all_environments():
        for k, v in env.items():
            if k in dom:
                assert dom[k][0] <= int(v) <= dom[k][1] and in_domain(k, int(v)) == int(v), (k, v)
            else:
                assert str(v) in ("0", "1"), (k, v)


# ---- the dispatcher of ptmi.hip against the instance table of the GPU file -----------------------------------------------------------------------------------

def _with_flags_calls(text):
    """{kernel named in the lambda: (number of its `auto` parameters, number of run-time flags passed)} of every with_flags(...) call."""
    calls = {}
    for m in re.finditer(r"with_flags\(\[\]\(([^)]*)\)\s*\{\s*return\s+&?([a-z_0-9]+)<[^}]*\}\s*,", text):
        n_auto = len(re.findall(r"\bauto\b", m.group(1)))
        depth, i, args = 1, m.end(), [""]
        while depth:  # the call's remaining arguments, split at top-level commas
            ch = text[i]
            depth += ch in "([{"
            depth -= ch in ")]}"
            if ch == "," and depth == 1:
                args.append("")
            elif depth:
                args[-1] += ch
            i += 1
        calls[m.group(2)] = (n_auto, len([a for a in args if a.strip()]))
    return calls


def test_the_instance_table_has_a_row_for_every_instance_the_dispatcher_can_return():
    import itertools

    import test_tuning_invariance_gpu as T

    text = open(os.path.join(CSRC, "ptmi.hip")).read()
    calls = _with_flags_calls(text)
    for kernel, flags in (("k_bvh2", T.BVH_FLAGS), ("shade_kernel", T.SHADE_FLAGS), ("tail_kernel", T.TAIL_FLAGS)):
        assert kernel in calls, (kernel, sorted(calls))
        assert calls[kernel] == (len(flags), len(flags)), "%s: the dispatcher passes %r flags, the table of test_tuning_invariance_gpu.py knows %d (%s): add the new flag's rows" % (
            kernel, calls[kernel], len(flags), ", ".join(flags))
    # the two selectors still fold the flags as the table assumes
    assert re.search(r"if constexpr \(!IS && !MULTI\) return &k_shade6<SORT, COUNT>;\s*else return &k_shade<IS, SORT, COUNT, MULTI>;", text)
    assert re.search(r"if constexpr \(SIX\) return &k_tail6<COUNT, NOABORT>;\s*else return &k_tail<IS, COUNT, MULTI, NOABORT>;", text)
    want = set()
    for cn, na in itertools.product((0, 1), repeat=2):
        want.add("k_bvh2<%d,%d>" % (cn, na))
        want.add("k_tail6<%d,%d>" % (cn, na))
    for is_, so, cn, mu in itertools.product((0, 1), repeat=4):
        want.add("k_shade6<%d,%d>" % (so, cn) if not is_ and not mu else "k_shade<%d,%d,%d,%d>" % (is_, so, cn, mu))
        want.add("k_tail<%d,%d,%d,%d>" % (is_, so, cn, mu))  # (k_tail's flags: IS, COUNT, MULTI, NOABORT — any four bits)
    rows = [r["instance"] for r in T.INSTANCES]
    assert len(want) == 40 and sorted(rows) == sorted(want)
