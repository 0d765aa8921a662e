"""The launch sequence of the training-side relative attention, pinned on the host.

csrc/rel_attention_run.cpp is pure host code.  tests/attention_plan_tracer.cpp links it against recording stubs and
prints, for every enumerated case (entry point, head_dim, precision, mask, table, channels per event, the block and tail
boundaries of the sequence lengths, batch and heads, strides, kept logits, workspaces, knobs, the GEMM back end's answer,
the CU count, refused calls), the return code, the number of launches, a digest of the size query and of every launch's
arguments, and the launches per launcher.  tests/attention_plan_trace.txt is that output; a change of
rel_attention_run.cpp that alters any launch of any case shows up here as a changed line, and
`attention_plan_tracer --dump CASE` from the two builds says what changed."""
import collections
import os
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "interactive-spectrogram-inpainting_amd" / "csrc"
ROCM = pathlib.Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
EXPECTED = ROOT / "tests" / "attention_plan_trace.txt"
# fields of a case id: entry/hd/p/m/d/t/c/s/b/h/q/l/w/k/g/u/r
F_ENTRY, F_HD, F_PREC, F_MASK, F_DENSE, F_TABLE, F_EVENTS, F_LEN, F_B, F_H, F_STRIDES, F_LOGITS, F_WS, F_KNOBS, F_GEMM, F_CUS, F_REFUSE = range(17)
LENGTHS = ["s8.8", "s128.128", "s129.129", "s256.256", "s257.257", "s258.258", "s259.259", "s1025.1025", "s4100.1025"]
COMMON_AXES = {F_HD: ["hd16", "hd32", "hd64", "hd48"], F_PREC: ["p0", "p1", "p2"], F_MASK: ["m0", "m1", "m2"], F_DENSE: ["d0", "d1"],
               F_TABLE: ["t0", "t1"], F_EVENTS: ["c1.1", "c4.1", "c1.4", "c4.4"], F_LEN: LENGTHS, F_B: ["b1", "b8"], F_H: ["h2", "h8"],
               F_STRIDES: ["q0", "q1"], F_LOGITS: ["l0", "l1", "l2"]}
AXES = {"f": {**COMMON_AXES, F_PREC: ["p0", "p1", "p2", "p3"], F_WS: ["w0", "w1", "w2", "w3", "w4"], F_KNOBS: ["k0", "k1", "k2"],
              F_CUS: ["u256", "u8"]},
        "b": {**COMMON_AXES, F_WS: ["w0", "w1"], F_KNOBS: ["k0", "k4", "k8", "k16"], F_GEMM: ["g0", "g1"]}}
Result = collections.namedtuple("Result", "rc launches digest kinds")


@pytest.fixture(scope="module")
def tracer(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    if not (ROCM / "include" / "hip" / "hip_runtime.h").exists():
        pytest.skip("no ROCm headers")
    exe = tmp_path_factory.mktemp("attention_plan") / "attention_plan_tracer"
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM / 'include'}", f"-I{ROOT / 'include'}",
                    f"-I{CSRC}", str(ROOT / "tests" / "attention_plan_tracer.cpp"), str(CSRC / "rel_attention_run.cpp"), "-o", str(exe)],
                   check=True)
    return exe


@pytest.fixture(scope="module")
def trace(tracer):
    return subprocess.run([str(tracer)], check=True, capture_output=True).stdout


@pytest.fixture(scope="module")
def cases(trace):
    """{case id: Result}"""
    out = {}
    for line in trace.decode().splitlines():
        if line.startswith("#"):
            continue
        cid, rc, n, digest, kinds = line.split()
        assert cid not in out
        kinds = {} if kinds == "-" else {k: int(v) for k, v in (kv.split(":") for kv in kinds.split(","))}
        out[cid] = Result(int(rc), int(n), digest, kinds)
    return out


def _with(cid, i, value):
    f = cid.split("/")
    return "/".join(f[:i] + [value] + f[i + 1:])


def _field(cid, i):
    return cid.split("/")[i]


def test_launch_sequence_is_the_committed_one(trace):
    expected = EXPECTED.read_bytes()
    if trace != expected:
        got, want = trace.decode().splitlines(), expected.decode().splitlines()
        changed = [g.split()[0] for g, w in zip(got, want) if g != w]
        pytest.fail(f"{len(changed)} changed lines ({len(got)} lines now, {len(want)} committed); first: {changed[:5]} "
                    "-- diff `attention_plan_tracer --dump CASE` of the two builds")


def test_case_count_is_the_stated_one(trace, cases):
    stated = [int(l.split()[2]) for l in trace.decode().splitlines() if l.startswith("# cases ")]
    assert stated == [len(cases)] and 300 < stated[0] < 1000


def test_every_accepted_call_launches_and_no_refused_call_does(cases):
    calls = {cid: res for cid, res in cases.items() if _field(cid, F_ENTRY) in "fb"}
    assert len(calls) > 300
    assert [cid for cid, res in calls.items() if res.rc == 0 and res.launches == 0] == []
    assert [cid for cid, res in calls.items() if res.rc != 0 and res.launches != 0] == []     # refusals precede all launches
    assert {res.rc for res in calls.values()} == {0, -1, -3, -4}                              # ISI_E_INVALID, _WORKSPACE, _UNSUPPORTED
    # every refusal of tests/test_attention_refusals.py and the tracer's further ones is refused
    assert [cid for cid, res in calls.items() if _field(cid, F_REFUSE) != "r0" and res.rc == 0] == []
    # a size query launches nothing
    assert all(res.launches == 0 for cid, res in cases.items() if _field(cid, F_ENTRY) in ("fq", "bq"))


@pytest.mark.parametrize("entry", ["f", "b"])
def test_every_axis_value_changes_some_trace(cases, entry):
    """A value that changes no digest would mean that the tracer does not reach the route it switches: for every value of
    every axis some case must differ from the case that has another value there and is otherwise the same."""
    for axis, values in AXES[entry].items():
        groups = collections.defaultdict(dict)
        for cid, res in cases.items():
            if _field(cid, F_ENTRY) == entry:
                groups[_with(cid, axis, "*")][_field(cid, axis)] = res.digest
        moved = set()
        for members in groups.values():
            moved |= {v for v, d in members.items() if any(d2 != d for d2 in members.values())}
        assert [v for v in values if v not in moved] == [], f"axis {axis} of {entry}"


def test_backward_takes_precision_3_like_precision_1(cases):
    """isi_rel_attention_bwd_f32 reads the precision as `>= 1` (split kernels, three-term GEMMs) and `== 2` (single-term
    products) only: mode 3's backward runs three-term products, launch for launch the calls of mode 1."""
    pairs = [(res, cases[_with(cid, F_PREC, "p1")]) for cid, res in cases.items()
             if _field(cid, F_ENTRY) == "b" and _field(cid, F_PREC) == "p3"]
    assert len(pairs) >= 8 and all(a == b for a, b in pairs)


def test_a_workspace_of_the_queried_size_is_accepted_and_one_unit_less_is_refused(cases):
    fwd = [(cid, res) for cid, res in cases.items() if _field(cid, F_ENTRY) == "f" and _field(cid, F_WS) == "w4" and "attn_fwd3" in res.kinds]
    assert len(fwd) >= 2
    for cid, res in fwd:
        short = cases[_with(cid, F_WS, "w2")]
        assert res.rc == 0 and (short.rc, short.launches) == (-1, 0), cid
    bwd = [(cid, res) for cid, res in cases.items() if _field(cid, F_ENTRY) == "b" and _field(cid, F_WS) == "w1"]
    assert len(bwd) >= 2
    for cid, res in bwd:
        assert (res.rc, res.launches) == (-3, 0) and cases[_with(cid, F_WS, "w0")].rc == 0, cid


@pytest.mark.parametrize("entry,tail", [("f", "attn_fwd_tail_rows"), ("b", "attn_bwd_tails")])
@pytest.mark.parametrize("low,high", [("s256.256", "s257.257"), ("s258.258", "s259.259")])
def test_tail_boundaries_change_the_kernels_unmasked_only(cases, entry, tail, low, high):
    """One or two rows beyond two or more full blocks go to the one-row kernels, three get a block of their own; under a
    causal mask (and with a dense mask) the ragged block is kept."""
    unmasked = masked = 0
    for cid, res in cases.items():
        if _field(cid, F_ENTRY) != entry or _field(cid, F_LEN) != low or res.rc or _field(cid, F_PREC) == "p0":
            continue
        other = cases.get(_with(cid, F_LEN, high))
        if other is None or other.rc:
            continue
        if _field(cid, F_MASK) == "m0" and _field(cid, F_DENSE) == "d0":
            assert (tail in res.kinds) != (tail in other.kinds) and (tail in other.kinds) == (high == "s257.257"), cid
            unmasked += 1
        else:
            assert set(res.kinds) == set(other.kinds) and tail not in res.kinds, cid
            masked += 1
    assert unmasked and masked


def test_g_from_kv_runs_the_key_kernel_the_tails_then_the_query_kernel(tracer, cases):
    picked = [cid for cid, res in cases.items() if res.kinds.get("attn_bwd_split") == 2]
    assert picked and all(_field(cid, F_LOGITS) == "l1" and not int(_field(cid, F_KNOBS)[1:]) & 8 for cid in picked)
    with_tails = [cid for cid in picked if "attn_bwd_tails" in cases[cid].kinds]
    assert with_tails
    for cid in picked:
        dump = subprocess.run([str(tracer), "--dump", cid], check=True, capture_output=True).stdout.decode().splitlines()
        order = []
        for line in dump:
            if line.startswith("attn_bwd_split "):
                assert " g_from_kv=1 " in line
                order.append("split" + line.split(" which=")[1].split()[0])
            elif line.startswith("attn_bwd_tails "):
                order.append("tails")
        assert order == (["split1", "tails", "split2"] if cid in with_tails else ["split1", "split2"]), cid
    # without kept logits, or with ISI_ATTN_G_FROM_KV=0, one launcher call runs both kernels
    off = cases[_with(with_tails[0], F_KNOBS, "k8")]
    assert off.rc == 0 and off.kinds["attn_bwd_split"] == 1
