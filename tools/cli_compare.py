"""Two builds of flake_amd_cli over one list of command lines: for each line the exit status, stderr (argv[0] and the
output directory replaced), which files were written and their SHA-256 must agree.

    python tools/cli_compare.py OLD_CLI NEW_CLI [TABLE]

Prints (and writes to TABLE) one line per command: OLD's exit status, "same" or what differs, the command.  The FLAC
inputs of the --decode and --recode lines are what OLD wrote for the encoding lines, plus one file with a flipped bit
and one cut inside its last frame.  Every command is a child with a time limit; the run stops at the first one that a
signal or the limit ends.  Exit status 0 only when every line says "same".  Needs a GPU."""
import hashlib
import os
import shutil
import subprocess
import sys
import tempfile

LIMIT = 120


def commands(src):
    """(name, environment, arguments); @OUT@ stands for the binary's own output directory, SRC/ for the shared inputs."""
    cmds = []
    for level in (2, 5, 10):
        for tag, extra in (("", []), ("b", ["-b", "1024"]), ("v", ["--verify"]), ("bv", ["-b", "1024", "--verify"])):
            cmds.append((f"enc{level}{tag}", {}, [f"-{level}", "--synth", "4", *extra, f"@OUT@/enc{level}{tag}.flac"]))
    for level in (5, 10):
        cmds.append((f"set{level}", {}, [f"-{level}", "--set", f"@OUT@/set{level}", "--synth-streams", "3", "--synth", "3"]))
    files = [f"{src}/{f}" for f in ("enc2.flac", "enc5b.flac", "enc10.flac", "set5/stream00001.flac", "set10/stream00002.flac",
                                    "flip.flac", "cut.flac")]
    for leg, env in (("dev", {}), ("host", {"FLAKE_AMD_INDEX_HOST": "1"})):
        for f in files:
            base = os.path.basename(f)[:-5]
            cmds.append((f"dec_{base}_{leg}", env, ["--decode", f, f"@OUT@/dec_{base}_{leg}.wav"]))
        cmds.append((f"decset_{leg}", env, ["--decode", "--set", f"@OUT@/decset_{leg}", *files]))
        cmds.append((f"decwin_{leg}", env, ["--decode", "--set", f"@OUT@/decwin_{leg}", "--skip", "1000", "--until", "9000", *files]))
        cmds.append((f"rec8_{leg}", env, ["-8", "--recode", "--set", f"@OUT@/rec8_{leg}", *files]))
        cmds.append((f"rec10v_{leg}", env, ["-10", "--verify", "--recode", "--set", f"@OUT@/rec10v_{leg}", *files]))
    return cmds


def tree(root):
    found = {}
    for d, _, names in os.walk(root):
        for f in names:
            p = os.path.join(d, f)
            found[os.path.relpath(p, root)] = hashlib.sha256(open(p, "rb").read()).hexdigest()
    return found


def run(exe, out, env, args):
    """(exit status, stderr, files written) of one command; the directories a --set line names are made first."""
    argv = [a.replace("@OUT@", out) for a in args]
    for a, b in zip(argv, argv[1:]):
        if a == "--set":
            os.makedirs(b, exist_ok=True)
    before = tree(out)
    e = {k: v for k, v in os.environ.items() if k != "FLAKE_AMD_INDEX_HOST"}
    e.update(env)
    try:
        p = subprocess.run([exe, *argv], capture_output=True, text=True, timeout=LIMIT, env=e)
    except subprocess.TimeoutExpired:
        return -1, "time limit", {}
    after = tree(out)
    return p.returncode, p.stderr.replace(exe, "CLI").replace(out, "OUTDIR"), {k: v for k, v in after.items() if before.get(k) != v}


def faulted(result):
    return result[0] < 0 or "illegal memory access" in result[1]


def main():
    old, new = os.path.abspath(sys.argv[1]), os.path.abspath(sys.argv[2])
    table = open(sys.argv[3], "w") if len(sys.argv) > 3 else None
    top = tempfile.mkdtemp(prefix="cli_compare_")
    outs = {}
    for who in ("old", "new", "src"):
        outs[who] = os.path.join(top, who)
        os.makedirs(outs[who])
    src, bad, made = outs["src"], 0, False
    for name, env, args in commands(src):
        if args[0] == "--decode" and not made:
            # the shared inputs: OLD's encodings, one with a bit flipped in the middle of its frames, one cut short
            made = True
            for f in tree(outs["old"]):
                os.makedirs(os.path.dirname(os.path.join(src, f)), exist_ok=True)
                open(os.path.join(src, f), "wb").write(open(os.path.join(outs["old"], f), "rb").read())
            whole = bytearray(open(os.path.join(src, "enc5.flac"), "rb").read())
            open(os.path.join(src, "cut.flac"), "wb").write(whole[:-9])
            whole[42 + (len(whole) - 42) // 2] ^= 0x20
            open(os.path.join(src, "flip.flac"), "wb").write(whole)
        a = run(old, outs["old"], env, args)
        b = run(new, outs["new"], env, args) if not faulted(a) else a
        diff = [what for what, x, y in zip(("status", "stderr", "files"), a, b) if x != y]
        if diff and a[2].keys() == b[2].keys():
            diff = [d.replace("files", "file contents") for d in diff]
        line = "%3d  %-28s %s%s" % (a[0], "same" if not diff else "DIFFERENT: " + ", ".join(diff),
                                    "".join(f"{k}={v} " for k, v in env.items()), " ".join(args).replace(src + "/", "SRC/").replace("@OUT@", "OUT"))
        print(line, flush=True)
        if table:
            table.write(line + "\n")
            table.flush()
        if diff:
            bad += 1
            print("  old:", a[0], repr(a[1]), sorted(a[2]), "\n  new:", b[0], repr(b[1]), sorted(b[2]), flush=True)
        if faulted(a) or faulted(b):
            print("a command was ended by a signal or the time limit, or met a device fault: stopping", flush=True)
            return 1
    if not bad:
        shutil.rmtree(top)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
