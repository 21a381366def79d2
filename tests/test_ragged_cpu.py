"""Ragged batches, the parts that need no GPU: the new entries are declared in the headers, exported by the
libraries and known to the Python view, and the comparison switch is documented where callers read."""
import os
import re

import flake_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ABI = ("fhip_frames_packed_upload_ragged", "fhip_frames_packed_begin_ragged", "fhip_md5_update_uploaded_ragged",
       "fhip_verify_frames_ragged_dev", "fhip_verify_frames_ragged")


def test_abi_entries_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "flakehip.h")).read()
    lib = flake_amd.load_library()
    for name in ABI:
        assert re.search(r"FHIP_API\s+int\s+" + name + r"\s*\(", text), name
        assert name in flake_amd.ABI_SYMBOLS
        assert getattr(lib, name).argtypes is not None
    # a null handle is refused, nothing is dereferenced
    assert lib.fhip_frames_packed_begin_ragged(None, None, None, None) == flake_amd.E_INVALID
    assert lib.fhip_frames_packed_upload_ragged(None, None, None) == flake_amd.E_INVALID
    assert lib.fhip_md5_update_uploaded_ragged(None, None, 0, 0, None, None, None) == flake_amd.E_INVALID
    assert lib.fhip_verify_frames_ragged(None, None, None, None, None) == flake_amd.E_INVALID


def test_host_entry_declared_exported_and_documented():
    text = open(os.path.join(ROOT, "include", "flake_amd.h")).read()
    assert re.search(r"FLAKE_AMD_API\s+long long\s+flake_amd_set_encode_ragged\s*\(", text)
    assert "FLAKE_AMD_SET_RAGGED" in text
    host = flake_amd.load_host_library()
    assert host.flake_amd_set_encode_ragged.restype is not None
    assert host.flake_amd_set_encode_ragged(None, None, 4, 0, None, None, None, 0, None) == -1
    assert hasattr(flake_amd.StreamSet, "encode_ragged")
