"""The operation records against the step plan: tests/records_model.hip, a host-only program with the whole text of
phyml_amd/csrc/phyhip_queue.hip compiled into it and linked in front of the built library (as the variants of
tests/unstored_model.py are), runs the two record encoders on an Instance built by hand and decodes what they wrote -- descriptor
records (IssueRec / ExecRec) and compact records (NtIssue / NtExec) -- back to a reach per child, a store bit and a step kind, which
must be the plan's (phyhip_step_plan.hpp).  No device is touched.  CPU-only."""
import os
import subprocess

import pytest

from unstored_model import CSRC, HIPCC, HOST_ONLY, LIBDIR, ROOT, needs_library

pytestmark = needs_library
LISTS_PER_SHAPE = 300
SHAPES = 11


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("records_model"))
    obj, exe = os.path.join(d, "records_model.o"), os.path.join(d, "records_model")
    unit = os.path.join(CSRC, "phyhip_queue.hip")
    subprocess.run([HIPCC] + HOST_ONLY + ['-DQUEUE_UNIT="%s"' % unit, "-c", "-o", obj, os.path.join(ROOT, "tests", "records_model.hip")],
                   check=True, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    # (the launch stubs' device code: an empty bundle the program defines -- it launches nothing)
    nm = subprocess.run(["nm", "-u", obj], check=True, stdout=subprocess.PIPE, text=True).stdout.split()
    fatbin = ["-Wl,--defsym=%s=records_model_no_kernels" % s for s in nm if s.startswith("__hip_fatbin")]
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-w", "-o", exe, obj] + fatbin + ["-L" + LIBDIR, "-lphyhip", "-Wl,-rpath," + LIBDIR],
                   check=True, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return exe


def test_both_encodings_say_what_the_plan_says(program):
    r = subprocess.run([program, "-", str(LISTS_PER_SHAPE)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0 and "RECORDS_MODEL OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    words = r.stdout.replace(",", "").split()
    fig = {k: int(words[words.index(k) + 1]) for k in ("lists", "descriptor_records", "compact_records", "pads", "unstored")}
    kinds = [int(x) for x in words[words.index("kinds") + 1:words.index("kinds") + 8]]
    assert fig["lists"] == SHAPES * LISTS_PER_SHAPE
    # (eight of the eleven shapes read compact records; every list of at least one operation, odd ones padded)
    assert fig["descriptor_records"] > fig["compact_records"] > fig["lists"] and fig["pads"] > 0 and fig["unstored"] > 0
    assert all(k > 0 for k in kinds[:7]), kinds
