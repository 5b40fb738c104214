"""lb::speculative_lattice (bioen_amd/csrc/lbfgs_state.hpp): the steps the host-driven log-weights engine evaluates in idle
batch slots are the ones the liblbfgs state machine asks for, bit for bit and where the order rules put them.

No GPU and no library: tests/spec_lattice_main.cpp is compiled with g++ from the header alone and run."""
import os
import re
import subprocess

from conftest import ROOT


def test_lattice_foresees_the_state_machine(tmp_path):
    """Scripted line searches for linesearch 1, 2 and 3 -- runs of "down", runs of "up", alternations, a first search with
    five "up", searches that walk out of the step bounds: after every rejection the step the machine asks for is the
    member of every list issued earlier in that search at the position the rules give; no step outside
    [min_step, max_step], none twice, never more than the capacity, and a smaller capacity is a prefix of a larger one."""
    exe = str(tmp_path / "spec_lattice")
    src = os.path.join(ROOT, "tests", "spec_lattice_main.cpp")
    build = subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-o", exe, src],
                           capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-3000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-3000:]
    m = re.search(r"(\d+) checks, 0 failures", run.stdout)
    assert m and int(m.group(1)) > 10000, run.stdout[-500:]
