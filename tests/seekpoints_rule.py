"""The seek-point rule of include/flake_amd.h restated on its own, for the tests of the recorder, of
flake_amd_seekpoints_of_frames and of the CLI: the targets are k * spacing; a block gets a point exactly when a target lies
in [first, first + samples), where `first` is the stream's sample count before it."""
import struct

PLACEHOLDER = (2 ** 64 - 1, 0, 0)


def rule(blocks, spacing):
    """blocks: (samples, bytes, samples of the block's first frame) in stream order.  The points as (sample, offset,
    frame_samples)."""
    pts, first, offset = [], 0, 0
    for samples, nbytes, first_frame in blocks:
        target = -(-first // spacing) * spacing            # the smallest target at or behind `first`
        if target < first + samples:
            pts.append((first, offset, first_frame))
        first += samples
        offset += nbytes
    return pts


def table(points):
    """A SEEKTABLE block's content."""
    return b"".join(struct.pack(">QQH", *p) for p in points)


def as_tuples(pts):
    return [(int(p["sample"]), int(p["offset"]), int(p["frame_samples"])) for p in pts]


def header_at(data, at):
    """(block size, coded number, blocking-strategy bit) of the frame header at data[at:], read field by field."""
    d = bytes(data[at:at + 16])
    assert d[0] == 0xFF and (d[1] & 0xFE) == 0xF8, "no frame header at a seek point"
    code, p = d[2] >> 4, 5
    ones = 0
    while (d[4] << ones) & 0x80:
        ones += 1
    number = d[4] & (0x7F >> ones) if ones else d[4]
    for _ in range(max(ones - 1, 0)):
        number = number << 6 | d[p] & 0x3F
        p += 1
    if code == 6:
        n = d[p] + 1
    elif code == 7:
        n = (d[p] << 8 | d[p + 1]) + 1
    else:
        n = 192 if code == 1 else 576 << (code - 2) if code <= 5 else 256 << (code - 8)
    return n, number, d[1] & 1


def metadata_blocks(data):
    """(blocks as (type, content), offset of the first frame) of a FLAC file's bytes; the last-block flag is held to
    stand on the last block and nowhere else."""
    assert data[:4] == b"fLaC"
    at, blocks = 4, []
    while True:
        last, kind, size = data[at] >> 7, data[at] & 0x7F, int.from_bytes(data[at + 1:at + 4], "big")
        blocks.append((kind, data[at + 4:at + 4 + size]))
        at += 4 + size
        if last:
            return blocks, at
        assert at < len(data), "no last metadata block"
