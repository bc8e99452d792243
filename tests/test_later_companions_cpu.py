"""The companion libraries added after the six of tests/test_companion_build_cpu.py, without a GPU.  That file pins its
tables to exactly six names, so a later companion stands in tables of its own (__graft_entry__.LATER_COMPANIONS,
api.LATER_COMPANIONS, api.LATER_COMPANION_CLASSES); here is asserted of them everything that file asserts of the six."""
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
NAMES = ("zstd_dict_compress",)


def test_build_list_and_binding_table_name_the_same_directories(hc):
    assert sorted(entry.LATER_COMPANIONS) == sorted(NAMES) and len(entry.LATER_COMPANIONS) == len(NAMES)
    assert {spec.csrc_dir for spec in hc.api.LATER_COMPANIONS.values()} == set(NAMES) == set(hc.api.LATER_COMPANIONS)
    assert set(hc.api.LATER_COMPANION_CLASSES) == set(NAMES)
    assert not set(NAMES) & set(entry.COMPANIONS) and not set(NAMES) & set(hc.api.COMPANIONS)
    for name, spec in hc.api.LATER_COMPANIONS.items():
        assert os.path.isfile(os.path.join(CSRC, spec.csrc_dir, "Makefile")), name
        assert spec.path == os.path.join(ROOT, "hipcomp-core_amd", "lib", spec.lib)
        assert spec.lib == f"libhipcomp_{spec.csrc_dir}.so"     # (what companion.mk links from NAME)
        assert hc.api.companion_spec(name) is spec
    assert hc.api.companion_spec("zstd") is hc.api.COMPANIONS["zstd"]
    # build() builds them, after the six
    import inspect
    assert "COMPANIONS + LATER_COMPANIONS" in inspect.getsource(entry.build)


@pytest.mark.parametrize("name", NAMES)
def test_bindings_are_exactly_the_exports(hc, name):
    spec = hc.api.LATER_COMPANIONS[name]
    text = open(os.path.join(CSRC, spec.csrc_dir, "exports.map")).read()
    in_map = set(re.findall(r"(\w+);", text.split("global:")[1].split("local:")[0]))
    assert os.path.exists(spec.path), "run __graft_entry__.build()"
    out = subprocess.run(["nm", "-D", "--defined-only", spec.path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
    assert in_map and set(spec.sigs) == in_map == exported, (set(spec.sigs) ^ in_map, in_map ^ exported)
    lib = getattr(hc.api, f"{name}_library")()
    assert type(lib) is hc.api.LATER_COMPANION_CLASSES[name] and lib is hc.api.companion_library(name)
    for fn_name, argtypes in spec.sigs.items():
        fn = getattr(lib, fn_name)
        assert fn.restype is ctypes.c_int, fn_name
        assert fn.argtypes is not None and list(fn.argtypes) == list(argtypes) and len(argtypes) > 0, fn_name


@pytest.mark.parametrize("name", NAMES)
def test_missing_library_names_its_build_command(hc, name, tmp_path):
    with pytest.raises(ImportError) as e:
        hc.api.LATER_COMPANION_CLASSES[name](str(tmp_path / "absent.so"))
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
        text = "\n".join(code)
        for d in ("zstd", "zstd_compress", "zstd_dict", "deflate_compress"):   # the headers it shares, as dependencies too
            assert f"$(CSRC)/{d}" in text.split("HDRS")[0] and f"$(CSRC)/{d}/" in text.split("HDRS")[1], (name, d)


@pytest.mark.parametrize("name", NAMES)
def test_shipped_assembly_passed_the_hazard_guard(name):
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


def test_the_shared_encoder_header_is_a_dependency_of_both_kernels():
    """csrc/zstd_compress/zstd_encode.hiph is compiled into two libraries: both Makefiles rebuild on its change"""
    for name in ("zstd_compress", "zstd_dict_compress"):
        text = open(os.path.join(CSRC, name, "Makefile")).read()
        assert "zstd_compress/zstd_encode.hiph" in text and "zstd_dict_compress" in text, name
    assert "zstd_dict_compress/zstd_dict_codes.hpp" in open(os.path.join(CSRC, "zstd_compress", "Makefile")).read()
