"""rekey_rows.py OUT.json [--added NAME ...] [--changed NAME [NAME ...] --parent-asm DIR] [--remeasured PART.json]: carry the newest
profiles/rNN_rows.json over to a build that only ADDED kernel objects (csrc/NAME.hip), or changed objects that hold
none of the measured kernels, without measuring again.

bench.py attaches the committed rocprof rows to its result only on the build they were measured on (the ids of
bench.kernel_source_id / bench.device_asm_id).  A new kernel file changes both ids although no measured kernel
changed.  This script proves that from the build at hand (csrc/build/*.gfx950.s, which build() leaves there): the
device assembly of every object but the added ones must hash to the table's device_asm_sha16 -- the measured kernels
are the same code, instruction for instruction -- and only then writes the same rows under the new ids, saying so
in the table's "_how".  --changed NAME: the object's assembly differs from the table's build, and that is
allowed only where no kernel the rows name is defined in it (neither in this build's assembly of it nor in the
parent's); the parent build's assembly of it is read from DIR (its build/*.gfx950.s) so that the table's id can
still be reproduced from all objects but the added ones.  --remeasured PART.json: rows collected again on the build
at hand (scripts/collect_profiles.sh with ROWS=...; the part must carry this build's ids) replace the table's rows
of the same names, and only the kernels of the rows that are carried over must be absent from the changed objects.
Anything else (a changed measured kernel whose row was not collected again) is refused: collect again
(scripts/collect_profiles.sh)."""
import argparse
import glob
import hashlib
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--added", nargs="*", default=[])
ap.add_argument("--changed", nargs="*", default=[])
ap.add_argument("--parent-asm")
ap.add_argument("--remeasured")
a = ap.parse_args()
assert a.added or a.changed, "nothing added or changed: the newest table is this build's"
assert not a.changed or a.parent_asm, "--changed needs --parent-asm DIR"
part = json.load(open(a.remeasured)) if a.remeasured else {"rows": {}}
if a.remeasured:
    assert part.get("kernel_source_sha16") == bench.kernel_source_id() or part.get("device_asm_sha16") == bench.device_asm_id(), (
        "%s was not measured on the build at hand" % a.remeasured)

tables = sorted(glob.glob(os.path.join(ROOT, "profiles", "r??_rows.json")), reverse=True)
tables = [t for t in tables if os.path.abspath(t) != os.path.abspath(a.out)]
old = json.load(open(tables[0]))
files = sorted(glob.glob(os.path.join(ROOT, "hipcomp-core_amd", "csrc", "build", "*.gfx950.s")))
names = {os.path.basename(f).split(".")[0] for f in files}
assert set(a.added) <= names, "not built: %s" % sorted(set(a.added) - names)
h = hashlib.sha256()
for path in files:                       # (bench.device_asm_id over the objects the table's build had)
    if os.path.basename(path).split(".")[0] in a.added:
        continue
    h.update(os.path.basename(path).encode())
    name = os.path.basename(path).split(".")[0]
    with open(os.path.join(a.parent_asm, os.path.basename(path)) if name in a.changed else path, "rb") as f:
        text = f.read()
    h.update(re.sub(rb"__hip_cuid_[0-9a-f]+", b"__hip_cuid_X", text))
    if name in a.changed:   # none of the measured kernels lives here, before or after
        measured = {phase["kernel"].split("<")[0] for key, row in old["rows"].items() if key not in part["rows"]
                    for phase in row.values() if isinstance(phase, dict) and "kernel" in phase}
        with open(path, "rb") as f:
            both = text + f.read()
        hit = sorted(k for k in measured if re.search(rb"\b%s\b" % re.escape(k.encode()), both))
        assert not hit, "csrc/%s.hip defines measured kernels %s: collect again" % (name, hit)
same = h.hexdigest()[:16]
if same != old.get("device_asm_sha16"):
    sys.exit("%s was measured on assembly %s; the build at hand without %s has %s: a measured kernel changed, collect again"
             % (tables[0], old.get("device_asm_sha16"), a.added, same))
new = dict(old)
new["rows"] = dict(old["rows"])
new["rows"].update(part["rows"])
new["_how"] = old["_how"] + (
    "\nCarried over by scripts/rekey_rows.py from %s (sources %s, assembly %s): this build only added %s%s, and the "
    "device assembly of every other kernel object is that table's, instruction for instruction (checked from "
    "csrc/build/*.gfx950.s); %s." % (
        os.path.basename(tables[0]), old.get("kernel_source_sha16"), old.get("device_asm_sha16"),
        ", ".join("csrc/%s.hip" % n for n in a.added) or "nothing",
        " and changed %s, which holds none of the kernels of the rows carried over (checked against the parent build's "
        "assembly of it)" % ", ".join("csrc/%s.hip" % n for n in a.changed) if a.changed else "",
        "the rows %s were measured again on this build, nothing else was" % ", ".join(sorted(part["rows"]))
        if part["rows"] else "nothing was measured again"))
new["kernel_source_sha16"] = bench.kernel_source_id()
new["device_asm_sha16"] = bench.device_asm_id()
with open(a.out, "w") as f:
    json.dump(new, f, indent=1)
    f.write("\n")
print(a.out, new["kernel_source_sha16"], new["device_asm_sha16"])
