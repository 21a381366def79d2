"""Verification of stream sets, the parts that need no GPU: the new entries are exported with the prototypes the
ctypes view declares, the view routes frame_numbers= to them, and the CLI's usage text offers --verify with --set."""
import ctypes as C
import os
import re
import subprocess

import flake_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def test_abi_entries_and_prototypes():
    lib = flake_amd.load_library()
    vp, pin, pout = C.c_void_p, C.POINTER(flake_amd.VerifyIn), C.POINTER(flake_amd.VerifyOut)
    for name in ("fhip_verify_frames_numbered_dev", "fhip_verify_frames_numbered"):
        assert name in flake_amd.ABI_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == [vp, pin, vp, pout]
        # the header: (ctx, in, frame_numbers, out)
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, header("flakehip.h"))
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == 4 and args[2] == "const uint32_t *frame_numbers"
    assert list(lib.fhip_last_verify_failure.argtypes) == [vp, vp, vp]
    # null handles are errors, not crashes; the structs did not grow
    assert lib.fhip_verify_frames_numbered(None, None, None, None) == flake_amd.E_INVALID
    assert lib.fhip_verify_frames_numbered_dev(None, None, None, None) == flake_amd.E_INVALID
    assert lib.fhip_last_verify_failure(None, None, None) == flake_amd.E_INVALID
    assert C.sizeof(flake_amd.VerifyIn) == 56 and C.sizeof(flake_amd.VerifyOut) == 16


def test_host_entries_and_prototypes():
    lib = flake_amd.load_host_library()
    assert list(lib.flake_amd_set_enable_verify.argtypes) == [C.c_void_p, C.c_int]
    assert len(lib.flake_amd_set_last_verify_failure.argtypes) == 4
    h = header("flake_amd.h")
    assert re.search(r"int\s+flake_amd_set_enable_verify\s*\(\s*FlakeAmdSet \*g,\s*int on\s*\)", h)
    assert re.search(r"int\s+flake_amd_set_last_verify_failure\s*\(\s*const FlakeAmdSet \*g,\s*int \*stream,\s*"
                     r"unsigned \*frame_number,\s*int \*status\s*\)", h)
    assert lib.flake_amd_set_enable_verify(None, 1) == -1
    assert lib.flake_amd_set_last_verify_failure(None, None, None, None) == 0
    for name in ("set_verify", "last_verify_failure"):
        assert callable(getattr(flake_amd.StreamSet, name))
    assert "not offered for sets" not in open(os.path.join(ROOT, "include", "flake_amd.h")).read()


def test_view_takes_frame_numbers():
    import inspect
    for name in ("verify_frames", "verify_frames_dev"):
        sig = inspect.signature(getattr(flake_amd.Encoder, name))
        assert sig.parameters["frame_numbers"].default is None


def test_cli_usage_offers_verify_for_sets():
    cli = os.path.join(flake_amd.LIB_DIR, "flake_amd_cli")
    for argv in ([cli], [cli, "--set"]):
        r = subprocess.run(argv, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2
        lines = [ln for ln in r.stderr.splitlines() if "--set OUTDIR" in ln]
        assert lines and all("[--verify]" in ln for ln in lines), r.stderr
