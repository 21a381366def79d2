"""Stream sets with variable block size, the parts that need no GPU: the new entries are exported with the prototypes
the headers and the ctypes view declare, the flag has its value, null handles are errors and not crashes, and the
CLI's usage text still parses."""
import ctypes as C
import inspect
import os
import re
import subprocess

import flake_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", txt, flags=re.S)


def proto(name):
    m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, header("flakehip.h"))
    assert m, name
    return [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")]


def test_abi_entries_and_prototypes():
    lib = flake_amd.load_library()
    vp, i, i64 = C.c_void_p, C.c_int, C.c_int64
    pin, pout = C.POINTER(flake_amd.VerifyIn), C.POINTER(flake_amd.VerifyOut)
    want = {
        "fhip_encode_blocks_vbs_packed_numbered": (
            [vp, vp, i, i, vp, vp, i64, vp, vp, vp, C.POINTER(i64)],
            ["fhip_ctx *ctx", "const int32_t *pcm", "int nblocks", "int block_size", "const uint32_t *block_first",
             "uint8_t *out", "int64_t out_cap", "int32_t *block_bytes", "int32_t *block_frames",
             "int32_t *block_max_frame", "int64_t *out_bytes"]),
        "fhip_verify_frames_blocks": (
            [vp, pin, vp, i, i, pout],
            ["fhip_ctx *ctx", "const fhip_verify_in *in", "const uint32_t *block_first", "int nblocks",
             "int block_size", "const fhip_verify_out *out"]),
        "fhip_verify_frames_blocks_dev": (
            [vp, pin, vp, i, i, pout],
            ["fhip_ctx *ctx", "const fhip_verify_in *in", "const uint32_t *block_first", "int nblocks",
             "int block_size", "const fhip_verify_out *out"]),
        "fhip_set_block_numbering": ([vp, i], ["fhip_ctx *ctx", "int on"]),
        "fhip_last_verify_number": ([vp, C.POINTER(C.c_uint32)], ["const fhip_ctx *ctx", "uint32_t *number"]),
    }
    for name, (argtypes, args) in want.items():
        assert name in flake_amd.ABI_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
        assert proto(name) == args, name
    # null handles are errors, not crashes; the structs did not grow
    assert lib.fhip_encode_blocks_vbs_packed_numbered(None, None, 0, 0, None, None, 0, None, None, None, None) == flake_amd.E_INVALID
    assert lib.fhip_verify_frames_blocks(None, None, None, 0, 0, None) == flake_amd.E_INVALID
    assert lib.fhip_verify_frames_blocks_dev(None, None, None, 0, 0, None) == flake_amd.E_INVALID
    assert lib.fhip_set_block_numbering(None, 1) == flake_amd.E_INVALID
    assert lib.fhip_last_verify_number(None, None) == flake_amd.E_INVALID
    assert C.sizeof(flake_amd.VerifyIn) == 56 and C.sizeof(flake_amd.VerifyOut) == 16 and C.sizeof(flake_amd.Batch) == 104


def test_flag_and_host_entries():
    assert flake_amd.SET_VBS == 4
    h = header("flake_amd.h")
    assert re.search(r"#define\s+FLAKE_AMD_SET_VBS\s+4u", h)
    assert re.search(r"#define\s+FLAKE_AMD_SET_MD5_HOST\s+1u", h) and re.search(r"#define\s+FLAKE_AMD_SET_MD5_OFF\s+2u", h)
    lib = flake_amd.load_host_library()
    # a null `like` is refused with a message, whatever the flags
    assert lib.flake_amd_set_open(None, 4, flake_amd.SET_VBS) is None
    assert b"invalid parameters" in lib.flake_amd_set_last_error(None)
    assert lib.flake_amd_set_encode(None, None, 4, 0, 4096, None, None, 0, None) == -1
    assert lib.flake_amd_set_encode_ragged(None, None, 4, 0, None, None, None, 0, None) == -1
    assert "stays outside sets" not in open(os.path.join(ROOT, "include", "flake_amd.h")).read()


def test_flag_is_checked_before_any_device_is_touched():
    """The flag on a context without variable block size, and variable block size without the flag, are refused by
    flake_amd_set_open's argument checks: no GPU needed to see the messages."""
    lib = flake_amd.load_host_library()
    for level, flags, text in ((5, flake_amd.SET_VBS, b"FLAKE_AMD_SET_VBS"), (10, 0, b"variable block size"),
                               (10, 8, b"flags")):
        ctx = flake_amd.HostContext(channels=2, sample_rate=44100, bits_per_sample=16)
        ctx.params.compression = level
        assert lib.flake_amd_set_defaults(C.byref(ctx.params)) == 0
        assert lib.flake_amd_set_open(C.byref(ctx), 4, flags) is None
        assert text in lib.flake_amd_set_last_error(None), (level, flags)


def test_view_has_the_methods():
    for name in ("encode_blocks_vbs_packed_numbered", "verify_frames_blocks", "verify_frames_blocks_dev",
                 "set_block_numbering", "last_verify_failure"):
        assert callable(getattr(flake_amd.Encoder, name))
    sig = inspect.signature(flake_amd.Encoder.verify_frames_blocks)
    assert list(sig.parameters)[1:6] == ["stream", "frame_bytes", "pcm", "block_first", "block_size"]
    assert inspect.signature(flake_amd.StreamSet.__init__).parameters["flags"].default == 0


def test_cli_usage_still_parses():
    cli = os.path.join(flake_amd.LIB_DIR, "flake_amd_cli")
    for argv in ([cli], [cli, "--set"], [cli, "-10", "--set"]):
        r = subprocess.run(argv, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2
        lines = [ln for ln in r.stderr.splitlines() if "--set OUTDIR" in ln]
        assert lines and all("[--verify]" in ln and "[-0..-12]" in ln for ln in lines), r.stderr
