"""The launch sequence of the VQ-VAE forward, pinned on the host.

csrc/vqvae_run.cpp is pure host code.  tests/forward_plan_tracer.cpp links it against recording stubs and prints, for
every enumerated case (geometries, precisions, modes, outputs, knobs, denied kernel predicates, refused calls; a few
shapes folded into each), the return codes, the numbers of launches and a digest of the size query and of every
launch's arguments.  tests/forward_plan_trace.txt is that output; a change of vqvae_run.cpp that alters any launch of
any case shows up here as a changed line, and `forward_plan_tracer --dump CASE` from the two builds says what changed."""
import os
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
CSRC = ROOT / "interactive-spectrogram-inpainting_amd" / "csrc"
ROCM = pathlib.Path(os.environ.get("ROCM_PATH", "/opt/rocm"))
EXPECTED = ROOT / "tests" / "forward_plan_trace.txt"
KNOB_BITS = {1: "no_pairs", 2: "no_conv_first", 4: "no_vq_fusion", 8: "no_setup_fusion", 16: "no_code_tables"}
N_DENY_BITS = 9


@pytest.fixture(scope="module")
def trace(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    if not (ROCM / "include" / "hip" / "hip_runtime.h").exists():
        pytest.skip("no ROCm headers")
    exe = tmp_path_factory.mktemp("forward_plan") / "forward_plan_tracer"
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", f"-I{ROCM / 'include'}", f"-I{ROOT / 'include'}",
                    f"-I{CSRC}", str(ROOT / "tests" / "forward_plan_tracer.cpp"), str(CSRC / "vqvae_run.cpp"), "-o", str(exe)],
                   check=True)
    return subprocess.run([str(exe)], check=True, capture_output=True).stdout


def _cases(text):
    """{case id: ([return code per shape], [launches per shape], digest)}"""
    out = {}
    for line in text.decode().splitlines():
        if line.startswith("#"):
            continue
        cid, rcs, ns, digest = line.split()
        assert cid not in out
        out[cid] = ([int(v) for v in rcs.split(",")], [int(v) for v in ns.split(",")], digest)
    return out


def test_launch_sequence_is_the_committed_one(trace):
    expected = EXPECTED.read_bytes()
    if trace != expected:
        got, want = trace.decode().splitlines(), expected.decode().splitlines()
        changed = [g.split()[0] for g, w in zip(got, want) if g != w]
        pytest.fail(f"{len(changed)} changed lines ({len(got)} lines now, {len(want)} committed); first: {changed[:5]} "
                    "-- diff `forward_plan_tracer --dump CASE` of the two builds")


def test_every_accepted_call_launches_and_no_refused_call_does(trace):
    runs = [(cid, rc, n) for cid, (rcs, ns, _) in _cases(trace).items() for rc, n in zip(rcs, ns)]
    assert len(runs) > 1500
    assert [cid for cid, rc, n in runs if rc == 0 and n == 0] == []
    assert [cid for cid, rc, n in runs if rc != 0 and n != 0] == []      # refusals precede all launches
    assert {rc for _, rc, _ in runs} == {0, -1, -3}


@pytest.mark.parametrize("field,bits", [(7, sorted(KNOB_BITS)), (8, [1 << i for i in range(N_DENY_BITS)])], ids=["knobs", "deny"])
def test_every_axis_bit_changes_some_trace(trace, field, bits):
    """An axis that changes no digest would mean that the tracer does not reach the route it switches."""
    cases = _cases(trace)
    for bit in bits:
        moved = 0
        for cid, res in cases.items():
            f = cid.split("/")
            v = int(f[field][1:])
            if v & bit:
                partner = "/".join(f[:field] + [f[field][0] + str(v & ~bit)] + f[field + 1:])
                moved += partner in cases and cases[partner][2] != res[2]
        assert moved, f"bit {bit} of field {field} changes nothing"
