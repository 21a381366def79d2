"""`flake_amd_cli --recode --set`: three small FLAC files (fixed blocks, variable block size, fixed blocks) re-encoded at
level 8 in one run.  The outputs decode to the WAVs the sources decode to, their STREAMINFO digests are the sources',
and a source with a flipped bit is named, gets no output and makes the exit status non-zero while the other two files
are written."""
import os
import subprocess

import pytest
import torch as _torch

import flake_amd
from test_gpu_decode_set import FIXED_LENS, VBS_LENS, encode_set, flac_file, wav_data

pytestmark = pytest.mark.gpu

V = flake_amd
NAMES = ["a", "b", "c"]


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


@pytest.fixture(scope="module")
def picks():
    fixed = encode_set(FIXED_LENS[:5], 64, 5, 0, 100)
    return [fixed[0], encode_set(VBS_LENS[2:3], 256, 10, V.SET_VBS, 202)[0], fixed[4]]


def cli(*args):
    return subprocess.run([os.path.join(V.LIB_DIR, "flake_amd_cli"), *map(str, args)], capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("switches", [("-8",), ("-8", "-b", "96", "--verify"), ("-10",)])
def test_recode_set(picks, tmp_path, switches):
    for n, x in zip(NAMES, picks):
        flac_file(tmp_path / f"{n}.flac", x)
    out, wav = tmp_path / "out", tmp_path / "wav"
    out.mkdir(), wav.mkdir()
    p = cli(*switches, "--recode", "--set", out, *[tmp_path / f"{n}.flac" for n in NAMES])
    assert p.returncode == 0, p.stderr
    assert sorted(os.listdir(out)) == [f"{n}.flac" for n in NAMES]
    for n, x in zip(NAMES, picks):
        new = (out / f"{n}.flac").read_bytes()
        assert new[:8] == b"fLaC" + bytes([new[4], 0, 0, 34]) and (new[4] & 0x7F) == 0
        si, _ = V.read_streaminfo(new[8:42])
        assert bytes(si.md5sum) == bytes(x["si"].md5sum) and si.samples == len(x["pcm"]), n
        assert new[8:42] != x["si_bytes"]                           # other blocks, other frame sizes: a new STREAMINFO
        q = cli("--decode", out / f"{n}.flac", wav / f"{n}.wav")
        assert q.returncode == 0, q.stderr
        assert wav_data(wav / f"{n}.wav") == x["pcm"].astype("<i2").tobytes(), n


def test_recode_set_is_the_same_with_either_indexer(picks, tmp_path):
    """Blocks of 64, 256 and 64 are two index calls on the device, one call per file on the CPU: the same exit status,
    stderr and files.  A file cut inside its last frame is named by both and gets no output, its whole frames having
    gone through the set like everyone's."""
    names = []
    for n, x in zip(NAMES, picks):
        flac_file(tmp_path / f"{n}.flac", x)
        names.append(tmp_path / f"{n}.flac")
    x = picks[0]
    flac_file(tmp_path / "cut.flac", x, x["frames"][:len(x["frames"]) - 9])
    names.append(tmp_path / "cut.flac")
    runs = {}
    for leg, env in (("device", {}), ("host", {"FLAKE_AMD_INDEX_HOST": "1"})):
        e = {k: v for k, v in os.environ.items() if k != "FLAKE_AMD_INDEX_HOST"}
        e.update(env)
        out = tmp_path / f"out_{leg}"
        out.mkdir()
        p = subprocess.run([os.path.join(V.LIB_DIR, "flake_amd_cli"), "-8", "--recode", "--set", str(out), *map(str, names)],
                           capture_output=True, text=True, timeout=120, env=e)
        runs[leg] = (p.returncode, p.stderr.replace(str(out), "OUT"), [(f, (out / f).read_bytes()) for f in sorted(os.listdir(out))])
    assert runs["device"] == runs["host"]
    status, stderr, files = runs["device"]
    assert status == 1 and [f for f, _ in files] == [f"{n}.flac" for n in NAMES]
    cut = [ln for ln in stderr.splitlines() if "cut.flac" in ln]
    assert len(cut) == 1 and cut[0].endswith("the frame is cut or its CRC-16 fails"), stderr
    for n in NAMES:
        assert f"{n}.flac: {len(picks[NAMES.index(n)]['pcm'])} sample-frames -> " in stderr, stderr


def test_a_corrupt_source_is_named_and_the_others_are_written(picks, tmp_path):
    for n, x in zip(NAMES, picks):
        flac_file(tmp_path / f"{n}.flac", x)
    x = picks[1]
    bad = x["frames"].copy()
    bad[x["off"][2] + x["sizes"][2] // 2] ^= 0x20
    flac_file(tmp_path / "b.flac", x, bad)
    good, out = tmp_path / "good", tmp_path / "out"
    good.mkdir(), out.mkdir()
    (out / "b.flac").write_bytes(b"left over from an earlier run")
    assert cli("-8", "--recode", "--set", good, tmp_path / "a.flac", tmp_path / "c.flac").returncode == 0
    p = cli("-8", "--recode", "--set", out, *[tmp_path / f"{n}.flac" for n in NAMES])
    assert p.returncode != 0 and "b.flac" in p.stderr
    assert sorted(os.listdir(out)) == ["a.flac", "c.flac"]
    for n in ("a", "c"):
        assert (out / f"{n}.flac").read_bytes() == (good / f"{n}.flac").read_bytes(), n
    # a file of another format is an error that names it; no inputs is a usage error that says what is not carried
    mono = V.HostStreaminfo(min_block_size=64, max_block_size=64, sample_rate=44100, channels=1, bits_per_sample=16)
    (tmp_path / "m.flac").write_bytes(b"fLaC" + bytes([0x80, 0, 0, 34]) + V.write_streaminfo(mono))
    p = cli("-8", "--recode", "--set", out, tmp_path / "a.flac", tmp_path / "m.flac")
    assert p.returncode != 0 and "m.flac" in p.stderr and "format" in p.stderr
    p = cli("--recode", "--set", out)
    assert p.returncode == 2 and "metadata" in p.stderr
