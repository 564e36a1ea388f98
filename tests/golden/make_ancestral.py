#!/usr/bin/env python3
"""Regenerate tests/golden/ancestral_*.txt.gz: the `--ancestral` output of the REAL reference, run CPU-only.

Runs only where the reference sources exist and oracle/_ref/phyml_glue_driver has been built (the build container):
    python -c 'import __graft_entry__ as g; g.build()' && python tests/golden/make_ancestral.py
The two files are the reference's own *_phyml_ancestral_seq.txt, byte for byte under gzip (no name, no time stamp in the header), for the inputs make_golden.py::synth_inputs
regenerates and the model arguments make_golden.py gives the fixture of the same name -- data only, no reference source travels.
With --no_colalias site s is pattern s - 1, and NodeLabel is the node index of the .phyg dump.  The run's final lnL is checked
against the fixture's (manifest.json).
"""
import gzip
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import make_golden as mg  # noqa: E402

DRIVER = os.path.join(ROOT, "oracle", "_ref", "phyml_glue_driver")

# fixture: (synth_inputs arguments after the tag, driver options, model arguments of make_golden.py for that fixture)
CASES = {
    "synth_nt_300x40": ((300, 40, 4, 7, 0.05, 0.4), ["--gtr-rr", mg.GTR_RR], ["-d", "nt", "-m", "GTR", "-f", mg.NT_FREQ]),
    "synth_aa_90x24": ((90, 24, 20, 8, 0.05, 0.4), [], ["-d", "aa", "-m", "LG", "-f", "m"]),
}


def main():
    if not os.path.exists(DRIVER):
        raise SystemExit("build oracle/_ref first: __graft_entry__.build() where the reference sources exist")
    manifest = json.load(open(os.path.join(HERE, "manifest.json")))["lnL"]
    tmp = tempfile.mkdtemp(prefix="ancestral_")
    try:
        for name, (shape, dopts, margs) in CASES.items():
            ali, tre, _ = mg.synth_inputs(tmp, name, *shape)
            args = dopts + ["--", "-i", os.path.basename(ali), "-u", os.path.basename(tre)]   # (run inside tmp: no path in the output)
            args = args + margs + ["-c", "4", "-a", "1.0", "-o", "n", "-b", "0", "--no_colalias", "--ancestral"]
            r = subprocess.run([DRIVER] + args, cwd=tmp, env=dict(os.environ, GLUE_MODE="host"), stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, text=True)
            if r.returncode != 0:
                print(r.stdout[-3000:])
                raise SystemExit(f"driver failed: {name}")
            lnl = float(re.search(r'"lnL_final": (\S+?),', r.stdout).group(1))
            assert lnl == manifest[name], (name, lnl, manifest[name])
            out = os.path.join(HERE, "ancestral_" + name + ".txt.gz")
            with open(out, "wb") as f, gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0, compresslevel=9) as g:
                g.write(open(ali + "_phyml_ancestral_seq.txt", "rb").read())
            print(f"{name:20s} lnL={lnl!r}  {os.path.getsize(out) / 1024:.0f} KiB")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
