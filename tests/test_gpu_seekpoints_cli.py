"""`flake_amd_cli --seekpoints N` through the single-file encode, --set and --recode --set, and `--reseek N --set`: the
file is "fLaC", STREAMINFO, the SEEKTABLE, then what the same command writes without the switch; the table is the rule's
(seekpoints_rule.py) over the frames the CPU indexer finds; and the project's own seek path uses it: the window decode
indexes the four frames between two seek points instead of all thirty."""
import os
import subprocess

import pytest
import torch as _torch

import flake_amd
from seekpoints_rule import PLACEHOLDER, header_at, metadata_blocks, rule, table
from test_gpu_decode_set import encode_set, flac_file, wav_data
from test_gpu_decode_windows_cli import seek_file

pytestmark = pytest.mark.gpu

V = flake_amd
BS, FRAMES = 64, 30


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


def cli(*args):
    return subprocess.run([os.path.join(V.LIB_DIR, "flake_amd_cli"), *map(str, args)], capture_output=True, text=True, timeout=120)


def ok(*args):
    p = cli(*args)
    assert p.returncode == 0, p.stderr
    return p


def rule_of_file(data, spacing):
    """The rule's points over the frames of a FLAC file's bytes, each frame a block; and the number of frames."""
    blocks, at = metadata_blocks(data)
    si, _ = V.read_streaminfo(blocks[0][1])
    sizes, used = V.index_frames(si, data[at:])
    assert used == len(data) - at
    rows, pos = [], 0
    for n in sizes:
        rows.append((header_at(data, at + pos)[0], int(n), header_at(data, at + pos)[0]))
        pos += int(n)
    return rule(rows, spacing), len(sizes)


def frames_indexed(tmp_path, path, skip, until):
    """(frames decoded, frames indexed, the window's bytes) of a window decode of the file."""
    out = tmp_path / (os.path.basename(str(path)) + f".{skip}.wav")
    p = ok("--decode", "--skip", skip, "--until", until, path, out)
    line = [ln for ln in p.stderr.split("\n") if ln.endswith(" frames decoded") and " of " in ln][0].split()
    return int(line[0]), int(line[2]), wav_data(out)


def held(tmp_path, seeked, plain, spacing, placeholders=0):
    """`seeked` is `plain` with a SEEKTABLE behind STREAMINFO and nothing else changed; the table is the rule's; the file
    decodes; the window decode uses the table."""
    a, b = seeked.read_bytes(), plain.read_bytes()
    with_table, first_a = metadata_blocks(a)
    without, first_b = metadata_blocks(b)
    assert [k for k, _ in with_table] == [0, 3] + [k for k, _ in without[1:]] and 3 not in [k for k, _ in without]
    assert with_table[0] == without[0] and with_table[2:] == without[1:]            # STREAMINFO and the rest of the header
    assert a[first_a:] == b[first_b:]                                                # the frames
    want, nframes = rule_of_file(b, spacing)
    assert with_table[1][1] == table(want + [PLACEHOLDER] * placeholders)
    if spacing == 256:
        assert nframes == FRAMES
        whole = tmp_path / (seeked.name + ".whole.wav")
        ok("--decode", seeked, whole)                                                # (with its MD5 check)
        got = frames_indexed(tmp_path, seeked, 579, 704)
        ref = frames_indexed(tmp_path, plain, 579, 704)
        assert got[:2] == (2, 4) and ref[:2] == (2, FRAMES)
        assert got[2] == ref[2] == wav_data(whole)[4 * 579:4 * 704]
    return want


def test_single_file(tmp_path):
    plain = tmp_path / "plain.flac"
    ok("--synth", FRAMES, "-b", BS, plain)
    for spacing, placeholders in ((256, 0), (50, 9), (100000, 0)):
        out = tmp_path / f"seek{spacing}.flac"
        ok("--synth", FRAMES, "-b", BS, "--seekpoints", spacing, out)
        want = held(tmp_path, out, plain, spacing, placeholders)
        assert len(want) + placeholders == -(-FRAMES * BS // spacing)                # the reservation: ceil(samples / N)
    assert [k for k, _ in metadata_blocks(plain.read_bytes())[0]] == [0, 4, 1]       # STREAMINFO, vendor comment, padding


def test_single_file_level_10(tmp_path):
    """Variable block size: a point names the first frame of a block; the reservation leaves placeholders."""
    plain, out = tmp_path / "plain.flac", tmp_path / "seek.flac"
    ok("-10", "--synth", 6, "-b", 256, plain)
    ok("-10", "--synth", 6, "-b", 256, "--seekpoints", 100, out)
    a = out.read_bytes()
    blocks, first = metadata_blocks(a)
    assert a[first:] == plain.read_bytes()[metadata_blocks(plain.read_bytes())[1]:]
    pts, n = V.read_seektable(blocks[1][1])
    assert len(blocks[1][1]) == 18 * 16 and n == 6 and list(pts["sample"]) == [256 * k for k in range(6)]
    for p in pts:
        assert header_at(a, first + int(p["offset"]))[:2] == (int(p["frame_samples"]), int(p["sample"]))
    ok("--decode", out, tmp_path / "whole.wav")


NAMES = ["stream00000.flac", "stream00001.flac"]


@pytest.fixture(scope="module")
def set_files(tmp_path_factory):
    """Two synthetic streams through --set, without the switch and with it."""
    d = tmp_path_factory.mktemp("seekset")
    plain, seeked = d / "plain", d / "seeked"
    plain.mkdir(), seeked.mkdir()
    ok("--set", plain, "--synth-streams", 2, "--synth", FRAMES, "-b", BS)
    ok("--set", seeked, "--synth-streams", 2, "--synth", FRAMES, "-b", BS, "--seekpoints", 256)
    assert sorted(os.listdir(plain)) == sorted(os.listdir(seeked)) == NAMES
    return plain, seeked


def test_set(set_files, tmp_path):
    plain, seeked = set_files
    for n in NAMES:
        held(tmp_path, seeked / n, plain / n, 256)


def test_recode_set(set_files, tmp_path):
    """The recoded files keep seeking: the sources' tables are dropped with the other metadata, new ones are written."""
    sources = set_files[1]
    again, again_seeked = tmp_path / "again", tmp_path / "again_seeked"
    again.mkdir(), again_seeked.mkdir()
    ok("-5", "-b", BS, "--recode", "--set", again, *[sources / n for n in NAMES])
    ok("-5", "-b", BS, "--recode", "--set", again_seeked, "--seekpoints", 256, *[sources / n for n in NAMES])
    for n in NAMES:
        held(tmp_path, again_seeked / n, again / n, 256)


def test_reseek(tmp_path):
    a, b = encode_set([BS * FRAMES, BS * 7 + 5], BS, 5, 0, 300)
    src, out = tmp_path / "src", tmp_path / "out"
    src.mkdir(), out.mkdir()
    flac_file(src / "bare.flac", a)                      # STREAMINFO alone
    flac_file(src / "short.flac", b)
    seek_file(src / "inside.flac", a, shift=5)           # a table whose points lie inside frames
    ok("--synth", FRAMES, "-b", BS, src / "full.flac")   # STREAMINFO, vendor comment, padding
    # a SEEKTABLE that is the last block, behind a vendor comment: the comment becomes the last block
    vendor = bytes([4, 0, 0, 12]) + (4).to_bytes(4, "little") + b"test" + bytes(4)
    stale = table([(0, 0, BS), (BS * 5, 7, BS)])
    (src / "order.flac").write_bytes(b"fLaC" + bytes([0, 0, 0, 34]) + a["si_bytes"] + vendor + bytes([0x83]) +
                                     len(stale).to_bytes(3, "big") + stale + bytes(a["frames"]))
    names = ["bare", "short", "inside", "full", "order"]
    p = ok("--reseek", 256, "--set", out, *[src / f"{n}.flac" for n in names])
    assert "decoded" not in p.stderr
    assert sorted(os.listdir(out)) == sorted(f"{n}.flac" for n in names)
    for n in names:
        old, new = (src / f"{n}.flac").read_bytes(), (out / f"{n}.flac").read_bytes()
        old_blocks, old_first = metadata_blocks(old)
        new_blocks, new_first = metadata_blocks(new)
        assert new[new_first:] == old[old_first:], n                                 # the frames, byte for byte
        kept = [blk for blk in old_blocks if blk[0] != 3]
        assert new_blocks[0] == kept[0] and new_blocks[2:] == kept[1:] and new_blocks[1][0] == 3, n
        want, _ = rule_of_file(old, 256)
        assert new_blocks[1][1] == table(want), n
        if n in ("inside", "order"):
            ok("--decode", out / f"{n}.flac", tmp_path / f"{n}.wav")
    assert [k for k, _ in metadata_blocks((out / "full.flac").read_bytes())[0]] == [0, 3, 4, 1]
    assert [k for k, _ in metadata_blocks((out / "order.flac").read_bytes())[0]] == [0, 3, 4]
    # the table with points inside frames made the window decode index the whole file; the new one spares it
    assert frames_indexed(tmp_path, src / "inside.flac", 579, 704)[:2] == (2, FRAMES)
    spared = frames_indexed(tmp_path, out / "inside.flac", 579, 704)
    assert spared[:2] == (2, 4) and frames_indexed(tmp_path, out / "bare.flac", 579, 704) == spared
    assert spared[2] == a["pcm"].astype("<i2").tobytes()[4 * 579:4 * 704]
    # the same on the CPU indexer
    host = tmp_path / "host"
    host.mkdir()
    q = subprocess.run([os.path.join(V.LIB_DIR, "flake_amd_cli"), "--reseek", "256", "--set", str(host),
                        *[str(src / f"{n}.flac") for n in names]], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, FLAKE_AMD_INDEX_HOST="1"))
    assert q.returncode == 0, q.stderr
    for n in names:
        assert (host / f"{n}.flac").read_bytes() == (out / f"{n}.flac").read_bytes(), n


def test_reseek_names_a_file_whose_frames_end_early(tmp_path):
    a, b = encode_set([BS * 9, BS * 7 + 5], BS, 5, 0, 310)
    out = tmp_path / "out"
    out.mkdir()
    flac_file(tmp_path / "cut.flac", a, a["frames"][:len(a["frames"]) - 9])
    flac_file(tmp_path / "good.flac", b)
    p = cli("--reseek", 128, "--set", out, tmp_path / "cut.flac", tmp_path / "good.flac")
    assert p.returncode == 1 and len([ln for ln in p.stderr.splitlines() if "cut.flac" in ln]) == 1
    assert os.listdir(out) == ["good.flac"]
    assert metadata_blocks((out / "good.flac").read_bytes())[0][1][1] == table(rule_of_file((tmp_path / "good.flac").read_bytes(), 128)[0])
