"""What `flake_amd_cli` refuses before its first device call: usage errors, files that are missing or are no FLAC / WAV
files, sets of more than one format, two inputs with one output name, levels that do not exist.  For every such command
line the exit status and the WHOLE of stderr (argv[0] replaced by CLI) are held to literals, and nothing may be written.

Every row runs twice: through the built CLI, and through the same source built into a stand-alone program with
-fsanitize=address,undefined and started as an ordinary child -- a sanitizer or leak report changes stderr and the exit
status, so every way out of every mode has to release what it holds."""
import os
import subprocess

import pytest

import flake_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "flake_amd", "host", "flake_amd_cli.c")

SET_FORM = ("CLI [-0..-12] [-b blocksize] --set OUTDIR [--verify] (in1.wav in2.wav ... | --synth-streams S --synth FRAMES "
            "[--channels C] [--bps B])\n")
RECODE = ("usage: CLI [-0..-12] [-b blocksize] --recode --set OUTDIR [--verify] a.flac b.flac ...\n"
          "       (files of one format; only STREAMINFO is written: other metadata blocks are not carried over)\n")
USAGE = ("usage: CLI [-0..-12] [-b blocksize] [--verify] (in.wav | --synth FRAMES [--channels C] [--bps B]) out.flac\n"
         "       " + SET_FORM + RECODE)
DECODE = "usage: CLI --decode in.flac out.wav\n       CLI --decode --set OUTDIR a.flac b.flac ...\n"
SET = "usage: " + SET_FORM
MISSING = "%s: No such file or directory\n"
JUNK = "junk.flac: not a FLAC file (no fLaC marker followed by STREAMINFO)\n"
META = "meta.flac: metadata runs past the file\n"
FORMAT = "m.flac: its format (1 channels, 16 bits, 44100 Hz) differs from a.flac's: a %s set takes one format\n"
CLASH = "a.flac and sub/a.flac would both be written to out/a.%s\n"
BAD_WAV = "cannot read bad.wav as PCM WAV\n"

ROWS = [
    ("", 2, USAGE),
    ("in.wav", 2, USAGE),
    ("--decode a.flac", 2, DECODE),
    ("--decode nowhere.flac o.wav", 1, MISSING % "nowhere.flac"),
    ("--decode junk.flac o.wav", 1, JUNK),
    ("--decode meta.flac o.wav", 1, META),
    ("--decode --set out", 2, "--decode --set needs input files\n"),
    ("--decode --set out a.flac m.flac", 1, FORMAT % "decode"),
    ("--decode --set out a.flac sub/a.flac", 1, CLASH % "wav"),
    ("--decode --set out nowhere.flac junk.flac", 1, MISSING % "nowhere.flac" + JUNK),
    ("--decode --set out -8 meta.flac", 1, MISSING % "-8" + META),
    ("--recode --set out", 2, RECODE),
    ("--recode a.flac", 2, RECODE),
    ("-8 --recode --set out a.flac m.flac", 1, FORMAT % "recode"),
    ("--recode --set out a.flac sub/a.flac", 1, CLASH % "flac"),
    ("--recode --set out nowhere.flac", 1, MISSING % "nowhere.flac"),
    ("-99 --recode --set out a.flac", 1, ""),
    ("-99 --synth 2 o.flac", 1, ""),
    ("--recode --decode --set out a.flac m.flac", 1, MISSING % "--decode" + FORMAT % "recode"),
    ("--set out", 2, SET),
    ("-5 --set", 2, SET),
    ("--set out --synth-streams 2", 2, SET),
    ("--set out bad.wav", 1, BAD_WAV),
    ("bad.wav o.flac", 1, BAD_WAV),
]


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    d = tmp_path_factory.mktemp("refusals")
    (d / "sub").mkdir(), (d / "out").mkdir()

    def head(channels, last=0x80):
        si = flake_amd.HostStreaminfo(min_block_size=64, max_block_size=64, sample_rate=44100, channels=channels,
                                      bits_per_sample=16)
        return b"fLaC" + bytes([last, 0, 0, 34]) + flake_amd.write_streaminfo(si)

    (d / "a.flac").write_bytes(head(2))
    (d / "sub" / "a.flac").write_bytes(head(2))
    (d / "m.flac").write_bytes(head(1))
    (d / "junk.flac").write_bytes(b"RIFF" + bytes(100))
    (d / "meta.flac").write_bytes(head(2, last=0) + bytes([1, 0, 0, 50]) + bytes(10))
    (d / "bad.wav").write_bytes(b"nope")
    return d


@pytest.fixture(scope="module")
def sanitized(tmp_path_factory):
    exe = tmp_path_factory.mktemp("cli_san") / "flake_amd_cli_san"
    subprocess.run(["gcc", "-std=gnu99", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), SRC, "-o", str(exe), "-L", flake_amd.LIB_DIR, "-lflake_amd",
                    "-lflakehip", "-Wl,-rpath," + flake_amd.LIB_DIR, "-lm", "-lpthread"],
                   check=True, capture_output=True, timeout=120)
    return str(exe)


def refused(exe, work, args, status, stderr):
    p = subprocess.run([exe, *args.split()], cwd=work, capture_output=True, text=True, timeout=60)
    assert (p.returncode, p.stderr.replace(exe, "CLI")) == (status, stderr)
    assert p.stdout == ""
    assert os.listdir(work / "out") == [] and not (work / "o.wav").exists() and not (work / "o.flac").exists()


@pytest.mark.parametrize("args,status,stderr", ROWS, ids=[r[0] or "(none)" for r in ROWS])
def test_refusal(work, args, status, stderr):
    refused(os.path.join(flake_amd.LIB_DIR, "flake_amd_cli"), work, args, status, stderr)


@pytest.mark.parametrize("args,status,stderr", ROWS, ids=[r[0] or "(none)" for r in ROWS])
def test_refusal_under_the_sanitizers(work, sanitized, args, status, stderr):
    refused(sanitized, work, args, status, stderr)
