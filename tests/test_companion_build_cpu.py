"""The companion libraries of libhipcomp.so (lib/libhipcomp_<name>.so, csrc/<name>/) without a GPU: they are
described once for the build (csrc/companion.mk, __graft_entry__.COMPANIONS) and once for the binding
(api.COMPANIONS).  Here: the two descriptions agree with each other, with each exports.map and with what the built
libraries export; the one recipe still runs the hazard guard on the object it ships; and the kept device assembly
of every companion passes that guard."""
import ctypes
import glob
import os
import re
import subprocess
import sys

import pytest

import __graft_entry__ as entry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hipcomp-core_amd", "csrc")
HAZ = os.path.join(CSRC, "check_asm_hazards.py")
NAMES = ("deflate", "deflate_compress", "gzip", "zstd", "zstd_compress", "zstd_dict")


def test_build_list_and_binding_table_name_the_same_directories(hc):
    assert sorted(entry.COMPANIONS) == sorted(NAMES) and len(entry.COMPANIONS) == len(NAMES)
    assert {spec.csrc_dir for spec in hc.api.COMPANIONS.values()} == set(NAMES) == set(hc.api.COMPANIONS)
    assert set(hc.api.COMPANION_CLASSES) == set(NAMES)
    order = list(entry.COMPANIONS)   # gzip links the two Deflate libraries
    assert order.index("deflate") < order.index("gzip") and order.index("deflate_compress") < order.index("gzip")
    for name, spec in hc.api.COMPANIONS.items():
        assert os.path.isfile(os.path.join(CSRC, spec.csrc_dir, "Makefile")), name
        assert spec.path == os.path.join(ROOT, "hipcomp-core_amd", "lib", spec.lib)
        assert spec.lib == f"libhipcomp_{spec.csrc_dir}.so"     # (what companion.mk links from NAME)


@pytest.mark.parametrize("name", NAMES)
def test_bindings_are_exactly_the_exports(hc, name):
    spec = hc.api.COMPANIONS[name]
    text = open(os.path.join(CSRC, spec.csrc_dir, "exports.map")).read()
    in_map = set(re.findall(r"(\w+);", text.split("global:")[1].split("local:")[0]))
    assert os.path.exists(spec.path), "run __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", spec.path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert in_map and set(spec.sigs) == in_map == exported, (set(spec.sigs) ^ in_map, in_map ^ exported)
    lib = getattr(hc.api, f"{name}_library")()
    assert type(lib) is hc.api.COMPANION_CLASSES[name] and lib is hc.api.companion_library(name)
    for fn_name, argtypes in spec.sigs.items():
        fn = getattr(lib, fn_name)
        assert fn.restype is ctypes.c_int, fn_name
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes) and len(argtypes) > 0, fn_name


@pytest.mark.parametrize("name", NAMES)
def test_missing_library_names_its_build_command(hc, name, tmp_path):
    with pytest.raises(ImportError) as e:
        hc.api.COMPANION_CLASSES[name](str(tmp_path / "absent.so"))
    text = str(e.value)
    assert "absent.so is missing" in text and "There is no fallback path." in text
    assert re.search(r"`make -C hipcomp-core_amd/csrc/%s`" % name, text), text
    assert "__graft_entry__" in text


def test_each_makefile_is_its_own_settings_and_the_one_recipe():
    for name in NAMES:
        lines = open(os.path.join(CSRC, name, "Makefile")).read().splitlines()
        code = [l for l in lines if l.strip() and not l.startswith("#")]
        assert code[-1] == "include ../companion.mk", name
        assert re.fullmatch(r"NAME\s*:=\s*%s" % name, code[0]), name
        assert not any("$(HIPCC)" in l or "hipcc" in l for l in code), name       # no compile or link line
        assert not any(l.startswith("\t") or re.search(r":(?!=)", l) for l in code), name   # no rule at all
    assert "$(HIPCC) $(CXXFLAGS)" not in open(os.path.join(CSRC, "gzip", "Makefile")).read()


def test_recipe_runs_the_guard_on_the_object_it_ships():
    """What test_build_guards_cpu.py asserts of csrc/Makefile, of companion.mk's rule."""
    mk = open(os.path.join(CSRC, "companion.mk")).read()
    rule = mk[mk.index("$(OBJDIR)/%.hip.o:"):]
    rule = rule[:rule.index("$(OBJDIR)/%.cpp.o:")]
    assert "-save-temps=obj" in rule and "check_asm_hazards.py" in rule
    assert "$(HIPCC) $(CXXFLAGS)" in rule.split("\n")[2]          # the flags of every object, EXTRA included
    assert rule.index("check_asm_hazards.py $(OBJDIR)") < rule.index("mv $(OBJDIR)/$*_temps/$*.hip.o")
    assert rule.index("cp $(OBJDIR)/$*_temps/") < rule.index("rm -rf $(OBJDIR)/$*_temps")   # the assembly is kept
    assert "$(EXTRA)" in mk[mk.index("CXXFLAGS"):mk.index("OBJS")]
    assert "--version-script=$(SRCDIR)/exports.map" in mk


@pytest.mark.parametrize("name", NAMES)
def test_shipped_assembly_passed_the_hazard_guard(name):
    """companion.mk keeps the checked device assembly of the kernel object; the guard accepts it and reads
    compiler-scheduled code as hazard-free (its calibration)."""
    build = os.path.join(CSRC, name, "build")
    sources = sorted(glob.glob(os.path.join(CSRC, name, "*.hip")))
    assert [os.path.basename(s) for s in sources] == [f"{name}_kernels.hip"]
    asm = os.path.join(build, f"{name}_kernels.gfx950.s")
    obj = os.path.join(build, f"{name}_kernels.hip.o")
    assert os.path.exists(asm) and os.path.exists(obj), "companion.mk keeps the assembly next to the object: run build()"
    assert sorted(glob.glob(os.path.join(build, "*.gfx950.s"))) == [asm]
    assert abs(os.path.getmtime(obj) - os.path.getmtime(asm)) < 300   # same make rule, same compile
    r = subprocess.run([sys.executable, HAZ, asm], capture_output=True, text=True)
    assert r.returncode == 0 and "calibration" not in r.stderr, (asm, r.stderr[-500:])
