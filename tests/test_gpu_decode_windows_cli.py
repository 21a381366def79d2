"""`flake_amd_cli --decode [--set OUTDIR] --skip N --until N`: the WAV holds exactly the window.  The expected bytes are
slices of the WAV the same file decodes to without the two options.  One file carries a correct SEEKTABLE, written here in
front of the encoder's frames, one the same table with every point moved into the middle of a frame: indexing the piece
is refused there and the whole file is indexed instead, with the same output."""
import os
import struct
import subprocess

import numpy as np
import pytest
import torch as _torch

import flake_amd
from test_gpu_decode_set import encode_set, flac_file, wav_data

pytestmark = pytest.mark.gpu

V = flake_amd
BS = 64
LENS = [BS * 30 + 13, BS * 25]


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


def cli(*args):
    return subprocess.run([os.path.join(V.LIB_DIR, "flake_amd_cli"), *map(str, args)], capture_output=True, text=True, timeout=120)


def seek_file(path, x, every=4, shift=0):
    """x with a SEEKTABLE: a point every `every` frames (and two placeholders), each offset moved by `shift` bytes."""
    pts = b"".join(struct.pack(">QQH", k * BS, int(x["off"][k]) + (shift if k else 0), BS) for k in range(0, len(x["sizes"]), every))
    pts += struct.pack(">QQH", 2 ** 64 - 1, 0, 0) * 2
    with open(path, "wb") as f:
        f.write(b"fLaC" + bytes([0x00, 0, 0, 34]) + x["si_bytes"] + bytes([0x83]) + len(pts).to_bytes(3, "big") + pts + bytes(x["frames"]))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """a.flac and b.flac (fixed blocks of 64), v.flac (variable block size), s.flac (a with a SEEKTABLE), m.flac (a with
    seek points inside frames); and the bytes of the WAV each decodes to as a whole."""
    d = tmp_path_factory.mktemp("wincli")
    a, b = encode_set(LENS, BS, 5, 0, 300)
    v = encode_set([256 * 6 + 100], 256, 10, V.SET_VBS, 404)[0]
    flac_file(d / "a.flac", a), flac_file(d / "b.flac", b), flac_file(d / "v.flac", v)
    seek_file(d / "s.flac", a)
    seek_file(d / "m.flac", a, shift=5)
    whole = {}
    for n, x in (("a", a), ("b", b), ("v", v), ("s", a), ("m", a)):
        p = cli("--decode", d / f"{n}.flac", d / f"{n}_whole.wav")
        assert p.returncode == 0, p.stderr
        whole[n] = wav_data(d / f"{n}_whole.wav")
        assert whole[n] == x["pcm"].astype("<i2").tobytes()
    return d, whole


WINDOWS = [(100, 700), (0, 64), (1000, 0), (BS * 8, BS * 12), (1900, 5000), (5000, 0), (5000, 6000)]


@pytest.mark.parametrize("name", ["a", "v", "s", "m"])
def test_single_file(files, tmp_path, name):
    d, whole = files
    total = len(whole[name]) // 4
    for skip, until in WINDOWS:
        out = tmp_path / f"{name}_{skip}_{until}.wav"
        args = ["--skip", skip] + (["--until", until] if until else [])
        p = cli("--decode", *args, d / f"{name}.flac", out)
        assert p.returncode == 0, (skip, until, p.stderr)
        assert p.stderr.count("MD5") == 1 and "not checked" in p.stderr
        end = min(until, total) if until else total
        assert wav_data(out) == whole[name][4 * skip:4 * max(end, skip)], (skip, until)        # (behind the end: an empty WAV)
        hdr = out.read_bytes()[:44]
        assert struct.unpack("<I", hdr[40:44])[0] == 4 * max(end - skip, 0)
    # --until alone
    out = tmp_path / "until.wav"
    assert cli("--decode", "--until", 333, d / f"{name}.flac", out).returncode == 0
    assert wav_data(out) == whole[name][:4 * 333]


def test_the_seek_table_spares_frames(files, tmp_path):
    """The piece between two seek points is all that is indexed; with points inside frames the whole file is."""
    d, whole = files
    counts = {}
    for name in ("s", "m", "a"):
        p = cli("--decode", "--skip", BS * 9 + 3, "--until", BS * 11, d / f"{name}.flac", tmp_path / f"{name}.wav")
        assert p.returncode == 0, p.stderr
        assert wav_data(tmp_path / f"{name}.wav") == whole[name][4 * (BS * 9 + 3):4 * BS * 11]
        line = [ln for ln in p.stderr.split("\n") if ln.endswith(" frames decoded") and " of " in ln][0].split()
        counts[name] = (int(line[0]), int(line[2]))
    assert counts["s"] == (2, 4)                  # frames 9 and 10 of the four between the points at frames 8 and 12
    assert counts["m"] == counts["a"] == (2, 31)  # the fallback: every frame indexed, the same two decoded


def test_set(files, tmp_path):
    d, whole = files
    out = tmp_path / "out"
    out.mkdir()
    names = ["a", "b", "s", "m"]
    p = cli("--decode", "--set", out, "--skip", 130, "--until", 1650, *[d / f"{n}.flac" for n in names])
    assert p.returncode == 0, p.stderr
    assert p.stderr.count("MD5") == 1
    assert sorted(os.listdir(out)) == sorted(f"{n}.wav" for n in names)
    for n in names:
        assert wav_data(out / f"{n}.wav") == whole[n][4 * 130:4 * min(1650, len(whole[n]) // 4)], n
    # a window behind the end of the shorter file only
    out2 = tmp_path / "out2"
    out2.mkdir()
    p = cli("--decode", "--set", out2, "--skip", LENS[1] + 10, d / "a.flac", d / "b.flac")
    assert p.returncode == 0, p.stderr
    assert wav_data(out2 / "a.wav") == whole["a"][4 * (LENS[1] + 10):] and wav_data(out2 / "b.wav") == b""


def test_a_flipped_bit_inside_the_window_names_the_file(files, tmp_path):
    d, whole = files
    raw = bytearray((d / "a.flac").read_bytes())
    raw[42 + (len(raw) - 42) // 2] ^= 0x20
    (tmp_path / "flip.flac").write_bytes(raw)
    out = tmp_path / "out"
    out.mkdir()
    p = cli("--decode", "--set", out, "--skip", 64, "--until", 1800, tmp_path / "flip.flac", d / "b.flac")
    assert p.returncode == 1 and "flip.flac" in p.stderr
    assert wav_data(out / "b.wav") == whole["b"][4 * 64:4 * min(1800, LENS[1])]
    # ... and outside it nobody looks: the frames of the window are all that is decoded
    p = cli("--decode", "--skip", 0, "--until", 64, tmp_path / "flip.flac", tmp_path / "head.wav")
    assert p.returncode in (0, 1)                 # (the indexer may end at the broken frame: the file is named then)
    assert wav_data(tmp_path / "head.wav") == whole["a"][:4 * 64]
