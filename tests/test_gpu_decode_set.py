"""A decode set (flake_amd_decode_set_*, flake_amd.DecodeSet) and `flake_amd_cli --decode --set`: streams that two
stream sets encoded (fixed blocks at level 5, variable block size at level 10) come back through ONE decode set,
round-robin, in device batches small enough to cut runs; every stream's PCM is its input and its digest its
STREAMINFO's; one corrupt stream fails alone.  Every comparison is exact."""
import math
import os
import subprocess

import numpy as np
import pytest
import torch as _torch          # (the fixture below brings torch's runtime up before this module's first handle)

import flake_amd

pytestmark = pytest.mark.gpu

V = flake_amd
BATCH = 7
FIXED_LENS = [64 * 5 + 13, 64 * 3, 64 * 9 + 1, 64 * 1 + 63, 64 * 6 + 32, 64 * 2 + 5, 64 * 12, 64 * 4 + 17]
VBS_LENS = [256 * 3 + 100, 256 * 2, 256 * 5 + 9, 256 * 1 + 200]


@pytest.fixture(scope="module", autouse=True)
def torch():
    if not _torch.cuda.is_available():
        pytest.fail("no HIP device")
    return _torch


def encode_set(lens, bs, level, flags, seed):
    """Streams of lens[s] samples through one StreamSet: whole blocks round-robin, then every tail in one ragged call.
    Returns [(pcm, STREAMINFO, frame bytes, frame sizes)]."""
    S = len(lens)
    pcm = [np.ascontiguousarray(V.synth_pcm(1, n, 2, 16, first_frame=seed + s).reshape(-1, 2), np.int32) for s, n in enumerate(lens)]
    data = [[] for _ in range(S)]
    with V.StreamSet(S, level=level, flags=flags, block_size=bs) as st:
        blocks = [(j, s) for s in range(S) for j in range(lens[s] // bs)]
        blocks.sort()
        if blocks:
            buf = np.concatenate([pcm[s][j * bs:(j + 1) * bs] for j, s in blocks])
            out, sizes = st.encode(buf, bs, [s for _, s in blocks])
            at = 0
            for (j, s), n in zip(blocks, sizes):
                data[s].append(out[at:at + n])
                at += n
        tails = [(s, lens[s] % bs) for s in range(S) if lens[s] % bs]
        if tails:
            buf = np.concatenate([pcm[s][lens[s] - t:] for s, t in tails])
            out, sizes = st.encode_ragged(buf, [t for _, t in tails], [s for s, _ in tails])
            at = 0
            for (s, t), n in zip(tails, sizes):
                data[s].append(out[at:at + n])
                at += n
        infos = [st.streaminfo(s) for s in range(S)]
        si_bytes = [st.streaminfo_bytes(s) for s in range(S)]
    res = []
    for s in range(S):
        frames = np.concatenate(data[s])
        fs, used = V.index_frames(infos[s], frames)
        assert used == len(frames)
        res.append(dict(pcm=pcm[s], si=infos[s], si_bytes=si_bytes[s], frames=frames, sizes=fs,
                        off=np.concatenate([[0], np.cumsum(fs)]).astype(int)))
    return res


@pytest.fixture(scope="module")
def streams():
    return encode_set(FIXED_LENS, 64, 5, 0, 100) + encode_set(VBS_LENS, 256, 10, V.SET_VBS, 200)


def like_of(streams):
    return V.HostStreaminfo(min_block_size=16, max_block_size=256, sample_rate=44100, channels=2, bits_per_sample=16)


def round_robin(streams, per, skip=()):
    """[(stream, first frame, frames)]: `per` frames of every stream in turn until all are used up."""
    at = [0] * len(streams)
    runs = []
    while any(at[s] < len(streams[s]["sizes"]) for s in range(len(streams)) if s not in skip):
        for s, x in enumerate(streams):
            if s in skip or at[s] >= len(x["sizes"]):
                continue
            n = min(per, len(x["sizes"]) - at[s])
            runs.append((s, at[s], n))
            at[s] += n
    return runs


def as_call(streams, runs, frames=None):
    frames = frames or [x["frames"] for x in streams]
    return [(s, frames[s][streams[s]["off"][a]:streams[s]["off"][a + n]], streams[s]["sizes"][a:a + n]) for s, a, n in runs]


def total_samples(streams):
    return sum(len(x["pcm"]) for x in streams)


@pytest.mark.parametrize("flags", [0, V.SET_MD5_HOST, V.SET_MD5_OFF])
@pytest.mark.parametrize("sample_bytes", [4, 2])
def test_twelve_streams_in_one_call(streams, monkeypatch, flags, sample_bytes):
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(BATCH))
    runs = round_robin(streams, 3)
    nframes = sum(n for _, _, n in runs)
    assert max(np.bincount([s for s, _, _ in runs])) > 1 and nframes > 4 * BATCH      # several runs per stream, many batches
    with V.DecodeSet(like_of(streams), len(streams), flags) as ds:
        got = ds.decode_runs(as_call(streams, runs), total_samples(streams), sample_bytes)
        assert ds.device_batches() == math.ceil(nframes / BATCH)                          # not one per stream or per run
        per = [[] for _ in streams]
        for (s, _, _), part in zip(runs, got):
            assert part is not None
            per[s].append(part)
        for s, x in enumerate(streams):
            out = np.concatenate(per[s])
            assert out.dtype == (np.int16 if sample_bytes == 2 else np.int32)
            assert np.array_equal(out, x["pcm"]), s
            assert ds.failed(s) is None
            if flags & V.SET_MD5_OFF:
                assert ds.md5(s) is None and "no digest" in ds.last_error()
            else:
                assert ds.md5(s) == bytes(x["si"].md5sum), s


def test_numbering_and_hashes_carry_across_calls(streams, monkeypatch):
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(BATCH))
    runs = round_robin(streams, 2)
    with V.DecodeSet(like_of(streams), len(streams)) as ds:
        per = [[] for _ in streams]
        want_batches = 0
        for c0 in range(0, len(runs), 9):                     # nine runs a call: 18 frames or fewer, three batches
            call = runs[c0:c0 + 9]
            cap = sum(int(np.sum([256] * n)) for _, _, n in call)
            for (s, _, _), part in zip(call, ds.decode_runs(as_call(streams, call), cap)):
                per[s].append(part)
            want_batches += math.ceil(sum(n for _, _, n in call) / BATCH)
            if c0 == 0:
                ds.md5(0)                                      # an early request finalises a copy: the states go on
        assert ds.device_batches() == want_batches
        for s, x in enumerate(streams):
            assert np.array_equal(np.concatenate(per[s]), x["pcm"]) and ds.md5(s) == bytes(x["si"].md5sum), s


def test_one_flipped_bit_fails_one_stream(streams, monkeypatch):
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(BATCH))
    victim, vf = 2, 4
    x = streams[victim]
    bad = x["frames"].copy()
    bad[x["off"][vf] + x["sizes"][vf] // 2] ^= 0x08
    # what the single-stream entry says of the same bytes
    with V.Encoder(V.level_params(5, block_size=256, variable_block_size=0), max_frames=64) as enc:
        ok, _, _, recs, summ, _ = enc.decode_frames(bad, x["sizes"], len(x["pcm"]), False, 0)
    assert not ok and summ[2] == vf
    frames = [y["frames"] for y in streams]
    frames[victim] = bad
    runs = round_robin(streams, 3)
    with V.DecodeSet(like_of(streams), len(streams)) as ds:
        got = ds.decode_runs(as_call(streams, runs, frames), total_samples(streams))
        assert ds.failed(victim) == (vf, int(summ[3]))
        assert ds.md5(victim) is None
        per = [[] for _ in streams]
        for (s, a, n), part in zip(runs, got):
            if s == victim and a + n > vf:
                assert part is None                            # the failing run and the stream's later ones
            else:
                per[s].append(part)
        assert np.array_equal(np.concatenate(per[victim]), x["pcm"][:3 * 64])           # the run before stands
        for s, y in enumerate(streams):
            if s != victim:
                assert np.array_equal(np.concatenate(per[s]), y["pcm"]) and ds.md5(s) == bytes(y["si"].md5sum), s
                assert ds.failed(s) is None
        # a later call that names the failed stream is refused whole
        before = ds.device_batches()
        with pytest.raises(V.FlakeHipError):
            ds.decode_runs(as_call(streams, [(0, 0, 1), (victim, 0, 1)], frames), 512)
        assert "failed" in ds.last_error() and ds.device_batches() == before
        assert ds.failed(0) is None and ds.md5(0) == bytes(streams[0]["si"].md5sum)


def packed(enc, pcm, n, first):
    pcm = np.ascontiguousarray(pcm, np.int32)
    nf = pcm.size // (n * 2)
    fb = np.zeros(nf, np.int32)
    b = V.Batch()
    b.pcm, b.nframes, b.block_size, b.frame_bytes, b.first_frame_number = pcm.ctypes.data, nf, n, fb.ctypes.data, first
    cap = nf * enc.frame_stride(n) + 64
    out = np.zeros(cap, np.uint8)
    wrote = V.C.c_int64(0)
    assert enc.lib.fhip_encode_frames_packed(enc._h, V.C.byref(b), out.ctypes.data, cap, V.C.byref(wrote)) == 0
    return out[:wrote.value].copy(), fb


@pytest.mark.parametrize("batch", [3, 4, 64])
def test_a_short_frame_in_the_middle_fails_wherever_the_batches_are_cut(monkeypatch, batch):
    """Frames of 64, 64, 40, 64, 64 samples, numbered 0 .. 4: with three frames a batch the short one ends a segment,
    where the device lets a last frame be shorter; the set holds the stream's block size from segment to segment."""
    monkeypatch.setenv("FLAKE_AMD_BATCH", str(batch))
    with V.Encoder(V.level_params(5, block_size=64, variable_block_size=0), max_frames=8) as enc:
        a, fa = packed(enc, V.synth_pcm(2, 64, 2, 16, first_frame=1), 64, 0)
        s, fs_ = packed(enc, V.synth_pcm(1, 40, 2, 16, first_frame=2), 40, 2)
        c, fc = packed(enc, V.synth_pcm(2, 64, 2, 16, first_frame=3), 64, 3)
        good, fg = packed(enc, V.synth_pcm(3, 64, 2, 16, first_frame=4), 64, 0)
    frames, sizes = np.concatenate([a, s, c]), np.concatenate([fa, fs_, fc])
    with V.DecodeSet(like_of(None), 2) as ds:
        got = ds.decode_runs([(0, frames, sizes), (1, good, fg)], 8 * 64)
        assert got[0] is None and ds.failed(0) is not None and ds.failed(0)[1] == V.V_NUMBER
        assert ds.failed(0)[0] in (2, 3)          # the short frame where the device sees its successor, else the frame behind it
        assert ds.failed(0)[0] == (3 if batch == 3 else 2)
        assert ds.failed(1) is None and len(got[1]) == 3 * 64
    # the short frame as the stream's last is fine, wherever the cut falls
    with V.DecodeSet(like_of(None), 1) as ds:
        got = ds.decode_runs([(0, np.concatenate([a, s]), np.concatenate([fa, fs_]))], 8 * 64)
        assert ds.failed(0) is None and len(got[0]) == 168


def test_a_broken_first_header_gets_the_device_status(streams):
    """The CRC-8 byte of a stream's very first header: the CPU parser cannot start the stream from it, and the status is
    still the one any later frame would get."""
    x = streams[1]
    bad = x["frames"].copy()
    fr = bad[:x["sizes"][0]]
    p = 4 + 1 + {6: 1, 7: 2}.get(int(fr[2]) >> 4, 0) + {12: 1, 13: 2, 14: 2}.get(int(fr[2]) & 15, 0)      # frame number 0: one byte
    bad[p] ^= 0x04
    with V.DecodeSet(like_of(streams), 2) as ds:
        got = ds.decode_runs([(0, bad, x["sizes"]), (1, streams[3]["frames"], streams[3]["sizes"])], 2048)
        assert got[0] is None and ds.failed(0) == (0, V.V_CRC8)
        assert np.array_equal(got[1], streams[3]["pcm"]) and ds.md5(1) == bytes(streams[3]["si"].md5sum)


def test_bad_arguments_change_nothing(streams):
    with V.DecodeSet(like_of(streams), 2) as ds:
        x = streams[0]
        for call in ([(2, x["frames"], x["sizes"])], [(-1, x["frames"], x["sizes"])],
                     [(0, x["frames"][:-5], x["sizes"])]):
            with pytest.raises(V.FlakeHipError):
                ds.decode_runs(call, len(x["pcm"]))
            assert ds.device_batches() == 0
        like24 = V.HostStreaminfo(min_block_size=16, max_block_size=256, sample_rate=44100, channels=2, bits_per_sample=24)
        with V.DecodeSet(like24, 1) as d24:
            with pytest.raises(V.FlakeHipError):
                d24.decode_runs([(0, x["frames"], x["sizes"])], len(x["pcm"]), sample_bytes=2)
        got = ds.decode_runs([(0, x["frames"], x["sizes"])], len(x["pcm"]))
        assert np.array_equal(got[0], x["pcm"]) and ds.md5(0) == bytes(x["si"].md5sum)
    with pytest.raises(V.FlakeHipError):
        V.DecodeSet(like_of(streams), 2, V.SET_MD5_HOST | V.SET_MD5_OFF)
    with pytest.raises(V.FlakeHipError):
        V.DecodeSet(like_of(streams), 2, V.SET_VBS)


def flac_file(path, x, frames=None):
    with open(path, "wb") as f:
        f.write(b"fLaC" + bytes([0x80, 0, 0, 34]) + x["si_bytes"] + bytes(x["frames"] if frames is None else frames))


def wav_data(path):
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[36:40] == b"data"
    return b[44:]


def test_cli_decode_set(streams, tmp_path):
    cli = os.path.join(V.LIB_DIR, "flake_amd_cli")
    names = ["a", "b", "c"]
    picks = [streams[0], streams[10], streams[4]]              # fixed, variable block size, fixed
    for n, x in zip(names, picks):
        flac_file(tmp_path / f"{n}.flac", x)
    one, many = tmp_path / "one", tmp_path / "many"
    one.mkdir(), many.mkdir()
    for n in names:
        subprocess.run([cli, "--decode", str(tmp_path / f"{n}.flac"), str(one / f"{n}.wav")], check=True, capture_output=True,
                       timeout=120)
    p = subprocess.run([cli, "--decode", "--set", str(many)] + [str(tmp_path / f"{n}.flac") for n in names],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr
    for n, x in zip(names, picks):
        assert wav_data(many / f"{n}.wav") == wav_data(one / f"{n}.wav") == x["pcm"].astype("<i2").tobytes(), n
    # one corrupt file: named, non-zero, and the others whole
    x = picks[1]
    bad = x["frames"].copy()
    bad[x["off"][2] + x["sizes"][2] // 2] ^= 0x20
    flac_file(tmp_path / "b.flac", x, bad)
    worse = tmp_path / "worse"
    worse.mkdir()
    p = subprocess.run([cli, "--decode", "--set", str(worse)] + [str(tmp_path / f"{n}.flac") for n in names],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "b.flac" in p.stderr
    assert all("sample-frames decoded" in ln for ln in p.stderr.splitlines() if "a.flac" in ln or "c.flac" in ln)
    for n in ("a", "c"):
        assert wav_data(worse / f"{n}.wav") == wav_data(one / f"{n}.wav"), n
    # a file of another format is an error that names it
    mono = V.HostStreaminfo(min_block_size=64, max_block_size=64, sample_rate=44100, channels=1, bits_per_sample=16)
    buf = (V.C.c_ubyte * 34)()
    V.load_host_library().flake_amd_write_streaminfo(V.C.byref(mono), buf)
    with open(tmp_path / "m.flac", "wb") as f:
        f.write(b"fLaC" + bytes([0x80, 0, 0, 34]) + bytes(buf))
    p = subprocess.run([cli, "--decode", "--set", str(worse), str(tmp_path / "a.flac"), str(tmp_path / "m.flac")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "m.flac" in p.stderr and "format" in p.stderr
    # a file that is missing and one that is no FLAC file are named and left out; the others are written in full
    (tmp_path / "junk.flac").write_bytes(b"RIFF" + bytes(100))
    rest = tmp_path / "rest"
    rest.mkdir()
    p = subprocess.run([cli, "--decode", "--set", str(rest), str(tmp_path / "nowhere.flac"), str(tmp_path / "a.flac"),
                        str(tmp_path / "junk.flac"), str(tmp_path / "c.flac")], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "nowhere.flac" in p.stderr and "junk.flac" in p.stderr
    for n in ("a", "c"):
        assert wav_data(rest / f"{n}.wav") == wav_data(one / f"{n}.wav"), n
    assert sorted(os.listdir(rest)) == ["a.wav", "c.wav"]
    # two inputs that would be written to the same file: refused before anything is written
    sub = tmp_path / "sub"
    sub.mkdir()
    flac_file(sub / "a.flac", picks[2])
    same = tmp_path / "same"
    same.mkdir()
    p = subprocess.run([cli, "--decode", "--set", str(same), str(tmp_path / "a.flac"), str(sub / "a.flac")],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and "both" in p.stderr and os.listdir(same) == []
