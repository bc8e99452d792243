"""The companion libraries of libhipcomp.so (lib/libhipcomp_<name>.so, csrc/<name>/) without a GPU: they are
described once for the build (csrc/companion.mk, __graft_entry__.COMPANIONS) and once for the binding
(api.COMPANIONS).  Here: the two descriptions agree with each other, with each exports.map and with what the built
libraries export; build() builds exactly the libraries of the table; the one recipe still runs the hazard guard on the
object it ships; the kept device assembly of every companion passes that guard; and every library is rebuilt when a
header that it includes changes, in whichever directory the header lies."""
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
NAMES = ("deflate", "deflate_compress", "gzip", "zstd", "zstd_compress", "zstd_dict", "zstd_dict_compress")


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


def test_build_makes_exactly_the_companions_of_the_table_in_its_order(monkeypatch):
    calls = []
    monkeypatch.setattr(entry, "_make", lambda *args: calls.append(args))
    entry.build()
    dirs = [args[args.index("-C") + 1] for args in calls]
    assert [os.path.basename(d) for d in dirs if os.path.dirname(d) == CSRC] == list(entry.COMPANIONS) == list(NAMES)
    assert dirs.index(CSRC) < dirs.index(os.path.join(CSRC, NAMES[0]))   # after the main library


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


# The headers each library is compiled from, by directory ("" is csrc/, "include" the public headers): the lists the
# Makefiles once kept by hand, less what no source of the library includes.  The Zstandard directories include each
# other's headers in both directions.
_COMMON = {"": ["wave_utils.hpp", "host_common.hpp"], "include": ["hipcomp.h", "hipcomp/shared_types.h"]}
_ZSTD_ENCODER = {"zstd": ["zstd_tables.hpp", "xxh64_math.hpp"], "deflate_compress": ["deflate_codes.hpp"],
                 "deflate": ["deflate_tables.hpp"], "zstd_dict": ["zstd_dict.hpp"],
                 "zstd_compress": ["zstd_codes.hpp", "zstd_compress_launch.hpp", "zstd_compress_sizing.hpp", "zstd_encode.hiph"],
                 "zstd_dict_compress": ["zstd_dict_codes.hpp"]}
_ZSTD_DECODER = {"": ["device_facts.hpp"], "zstd_dict": ["zstd_dict.hpp"],
                 "zstd": ["xxh64_math.hpp", "zstd_launch.hpp", "zstd_sizing.hpp", "zstd_tables.hpp", "zstd_decode.hiph"]}
REBUILT_BY = {
    "deflate": {"deflate": ["deflate_launch.hpp", "deflate_tables.hpp"]},
    "deflate_compress": {"deflate_compress": ["deflate_codes.hpp", "deflate_compress_launch.hpp"], "deflate": ["deflate_tables.hpp"]},
    "gzip": {"gzip": ["adler32_math.hpp", "gzip_frame.hpp", "gzip_launch.hpp"], "": ["crc32_math.hpp"],
             "include": ["hipcomp/deflate.h", "hipcomp/deflate_compress.h"]},
    "zstd": _ZSTD_DECODER,
    "zstd_compress": _ZSTD_ENCODER,
    "zstd_dict": {**_ZSTD_DECODER, "zstd_dict": ["zstd_dict.hpp", "zstd_dict_launch.hpp"]},
    "zstd_dict_compress": {**_ZSTD_ENCODER, "zstd_dict_compress": ["zstd_dict_codes.hpp", "zstd_dict_compress_launch.hpp"],
                           "include": ["hipcomp/zstd_compress.h"]},
}
NOT_REBUILT_BY = {name: {"zstd_dict_compress": ["zstd_dict_codes.hpp"], "zstd": ["zstd_tables.hpp"]}
                  for name in ("deflate", "deflate_compress", "gzip")}


def _paths(by_dir):
    return [os.path.join(ROOT, d, h) if d == "include" else os.path.join(CSRC, d, h) for d, hs in by_dir.items() for h in hs]


@pytest.mark.parametrize("name", NAMES)
def test_a_changed_header_rebuilds_exactly_the_libraries_that_include_it(name):
    """The dependencies come from the compiler (build/*.d, written by companion.mk's rules).  make -q says whether
    anything would be rebuilt (1) or not (0); -W takes a file as just changed and touches nothing."""
    def would_rebuild(*what_if):
        r = subprocess.run(["make", "-q", *what_if, "-C", os.path.join(CSRC, name)], capture_output=True, text=True)
        assert r.returncode in (0, 1), r.stderr[-500:]
        return r.returncode == 1

    assert not would_rebuild(), "a build() straight after build() compiles nothing: run build()"
    own = {"include": [f"hipcomp/{name}.h"], name: [f"{name}_kernels.hip", f"{name}_batch.cpp"]}
    for header in _paths(_COMMON) + _paths(own) + _paths(REBUILT_BY[name]):
        assert os.path.isfile(header) and would_rebuild("-W", header), (name, header)
    for header in _paths(NOT_REBUILT_BY.get(name, {})):
        assert os.path.isfile(header) and not would_rebuild("-W", header), (name, header)


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
    for r in (rule, mk[mk.index("$(OBJDIR)/%.cpp.o:"):mk.index("$(OUTDIR)/libhipcomp_$(NAME).so:")]):
        assert "-MMD" in r and "-MT $@" in r        # the compiler lists the headers of the object that ships
    assert mk.rstrip().endswith("-include $(OBJS:.o=.d)")
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
