"""The host layer's decoder (flake_amd_decode_*) and `flake_amd_cli --decode`: streams written by the host encoder come
back sample for sample, with the MD5 STREAMINFO carries."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import flake_amd

pytestmark = pytest.mark.gpu

CLI = os.path.join(flake_amd.LIB_DIR, "flake_amd_cli")


def encode_stream(level, bps, nblocks, tail, seed=0):
    """(params' block size, pcm [samples][2], stream bytes, STREAMINFO) from the host encoder."""
    with flake_amd.HostEncoder(level=level, bits_per_sample=bps) as he:
        n = he.ctx.params.block_size
        pcm = flake_amd.synth_pcm(nblocks + 1, n, 2, bps, first_frame=seed).reshape(-1, 2)[:nblocks * n + tail]
        stream, _ = he.encode_frames(pcm, n, tail)
        si = he.streaminfo()
        back, hi = flake_amd.read_streaminfo(flake_amd.write_streaminfo(si))
    return n, pcm, stream, back


@pytest.mark.parametrize("level,tail", [(5, 1000), (10, 0)])
@pytest.mark.parametrize("sample_bytes", [4, 2])
def test_host_decoder_round_trip(level, tail, sample_bytes):
    n, pcm, stream, si = encode_stream(level, 16, 6, tail, seed=level)
    got = flake_amd.index_frames(si, stream)
    assert got is not None
    sizes, used = got
    assert used == len(stream) and int(sizes.sum()) == len(stream)
    if level == 5:
        assert len(sizes) == 7
    half = len(sizes) // 2
    cut = int(sizes[:half].sum())
    with flake_amd.HostDecoder(si) as d:
        a = d.decode_frames(stream[:cut], sizes[:half], len(pcm), sample_bytes)
        b = d.decode_frames(stream[cut:], sizes[half:], len(pcm) - len(a), sample_bytes)
        out = np.concatenate([a, b])
        assert out.dtype == (np.int16 if sample_bytes == 2 else np.int32)
        assert np.array_equal(out, pcm.astype(out.dtype))
        assert d.md5() == bytes(si.md5sum) != bytes(16)
        # the numbers carry on across calls: the first half once more does not follow the second
        with pytest.raises(flake_amd.FlakeHipError) as e:
            d.decode_frames(stream[:cut], sizes[:half], len(pcm), sample_bytes)
        assert "NUMBER" in str(e.value) and "frame" in str(e.value)


def test_host_decoder_names_the_broken_frame():
    n, pcm, stream, si = encode_stream(5, 16, 5, 0)
    sizes, used = flake_amd.index_frames(si, stream)
    bad = stream.copy()
    bad[int(sizes[:3].sum()) + int(sizes[3]) // 2] ^= 0x40
    with flake_amd.HostDecoder(si) as d:
        with pytest.raises(flake_amd.FlakeHipError) as e:
            d.decode_frames(bad, sizes, len(pcm))
        assert "frame 3 " in str(e.value)


def write_wav(path, pcm, bps, rate=44100):
    ch = pcm.shape[1]
    nb = (bps + 7) // 8
    if nb == 2:
        data = pcm.astype("<i2").tobytes()
    else:
        raw = pcm.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :nb]
        data = raw.tobytes()
    hdr = b"RIFF" + struct.pack("<I", 36 + len(data)) + b"WAVEfmt " + struct.pack("<IHHIIHH", 16, 1, ch, rate,
                                                                                  rate * ch * nb, ch * nb, bps)
    with open(path, "wb") as f:
        f.write(hdr + b"data" + struct.pack("<I", len(data)) + data)
    return data


def wav_data(path):
    raw = open(path, "rb").read()
    at = raw.index(b"data")
    size = struct.unpack("<I", raw[at + 4:at + 8])[0]
    assert at + 8 + size == len(raw)
    return raw[at + 8:]


@pytest.mark.parametrize("level,bps", [(5, 16), (5, 24), (10, 16)])
def test_cli_decode_round_trip(tmp_path, level, bps):
    pcm = flake_amd.synth_pcm(5, 4096, 2, bps, first_frame=bps).reshape(-1, 2)[:4 * 4096 + 1234]
    wav, flac, back = (str(tmp_path / f) for f in ("in.wav", "a.flac", "b.wav"))
    data = write_wav(wav, pcm, bps)
    subprocess.run([CLI, f"-{level}", wav, flac], check=True, capture_output=True, timeout=120)
    r = subprocess.run([CLI, "--decode", flac, back], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert wav_data(back) == data
    if (level, bps) != (5, 16):
        return
    # one corrupted byte in the audio: a non-zero exit status, and the frame is named
    raw = bytearray(open(flac, "rb").read())
    raw[len(raw) * 2 // 3] ^= 0x08
    open(flac, "wb").write(bytes(raw))
    r = subprocess.run([CLI, "--decode", flac, back], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and re.search(r"frame \d+", r.stderr), r.stderr
