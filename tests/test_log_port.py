"""phyml_amd/csrc/phyhip_log.hpp -- the device's log() of the exact per-site route -- compiled by gcc for the host and held
against this image's libm, the one the reference calls (src/lk.c:854): the same double for every input tried, the near-1
branch, subnormals, zeros, negatives, infinities and NaNs included.  (The device runs the same header: its FMA and its plain
multiply / add are IEEE operations like the host's; tests/test_gpu_exact_site.py holds what the kernel makes of it to the
restatement's per-site arrays bit for bit.)"""
import os
import re
import struct
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "phyml_amd", "csrc", "phyhip_log.hpp")

SRC = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "%s"
static uint64_t s = 88172645463325252ull;
static uint64_t rnd(void) { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
int main(int argc, char **argv)
{
  long bad = 0, n = atol(argv[1]);
  for (long i = 0; i < n; ++i)
  {
    double x; const uint64_t r = rnd(); const double u = (double)(r >> 11) / 9007199254740992.0;
    switch (i & 7)
    {
      case 0: case 1: x = u; break;                                     /* (0,1): what a site likelihood is */
      case 2: x = ldexp(u, -(int)(r %% 1075)); break;                    /* ... scaled by 2^-k, k <= 1074: subnormals */
      case 3: case 4: x = 0.9 + 0.2 * u; break;                         /* both bounds of the near-1 branch */
      case 5: x = ldexp(1.0 + u, (int)(r %% 1024)); break;               /* [1, 2^1024) */
      case 6: x = ((r & 1) ? 1.0 - 0x1p-4 : 1.0 + 0x1.09p-4) + (u - 0.5) * 0x1p-40; break; /* right at those bounds */
      default: { uint64_t b = r; memcpy(&x, &b, 8); } break;            /* any bit pattern: negatives, infinities, NaNs */
    }
    if (i < 8) { const double sp[8] = {0.0, -0.0, 1.0, -1.0, 1.0 / 0.0, -1.0 / 0.0, 0x1p-1074, 0x1p-1022}; x = sp[i]; }
    const double a = log(x), b = phyhip_log_ref(x, phyhip_log_data);
    uint64_t ab, bb; memcpy(&ab, &a, 8); memcpy(&bb, &b, 8);
    if (ab != bb && !(a != a && b != b)) { if (bad < 10) printf("x=%%a libm=%%a port=%%a\n", x, a, b); ++bad; }
  }
  printf("%%ld inputs, %%ld differ\n", n, bad);
  return bad != 0;
}
"""


def test_the_port_is_this_libms_log(tmp_path):
    c = tmp_path / "t.c"
    c.write_text(SRC % HDR)
    exe = str(tmp_path / "t")
    subprocess.check_call(["gcc", "-O2", "-mfma", "-ffp-contract=off", "-o", exe, str(c), "-lm"])
    r = subprocess.run([exe, "40000000"], stdout=subprocess.PIPE, text=True)
    assert r.returncode == 0, r.stdout
    assert "40000000 inputs, 0 differ" in r.stdout


def test_the_table_is_the_one_in_libm():
    """ln2hi, ln2lo, poly[5], poly1[11] and the 128 {invc, logc} pairs of the header are ONE contiguous byte string of this
    image's libm.so.6: __log_data, first occurrence of its leading pair."""
    hdr = open(HDR).read()
    body = hdr[hdr.index("phyhip_log_data[274]"):]
    words = [int(x, 16) for x in re.findall(r"(0x[0-9a-f]+)ull", body[:body.index("};")])]
    assert len(words) == 274
    blob = b"".join(w.to_bytes(8, "little") for w in words)
    lib = None
    for p in ("/lib/x86_64-linux-gnu/libm.so.6", "/usr/lib/x86_64-linux-gnu/libm.so.6", "/lib64/libm.so.6"):
        if os.path.exists(p):
            lib = open(p, "rb").read()
            break
    assert lib is not None
    at = lib.find(blob)
    assert at > 0
    head = struct.pack("<2d", float.fromhex("0x1.62e42fefa3800p-1"), float.fromhex("0x1.ef35793c76730p-45"))
    assert lib.find(head) == at                    # __log_data starts at the first occurrence of {ln2hi, ln2lo}
    assert blob[:16] == head
    first = struct.unpack("<2d", blob[144:160])    # the table starts at byte +144
    assert first == (float.fromhex("0x1.734f0c3e0de9fp+0"), float.fromhex("-0x1.7cc7f79e69000p-2"))
