"""bin/chan_vese: what it answers, byte for byte, to the command lines that end before a device is touched -- the parser's own errors,
every refusal of the option checks and of the input loading, the rows where two refusals apply and the first one wins, and --help.

tests/golden/cli_refusals.json holds the command lines and the answers (exit status, stderr, stdout) of the binary as it was before the
command line was split into an options record and named stages; this test replays every row.  The rows name their files by
placeholder, and the test writes those files itself.  `python tests/test_cli_refusals.py BINARY` records the answers of BINARY for the
arguments the file already holds."""
import json
import os
import subprocess
import sys

import numpy as np

from cli_util import cli  # noqa: F401  (the fixture that builds the binary)

TABLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cli_refusals.json")


def write_inputs(tmp):
    """The files the rows refer to; returns placeholder -> path, longest path first so that answers map back without ambiguity."""
    ramp = (np.add.outer(np.arange(32), np.arange(32)) * 4).astype(np.uint8)
    files = {"{pgm}": "a.pgm", "{ppm}": "c.ppm", "{small}": "small.pgm", "{notpng}": "text.png", "{pgmpng}": "pgm.png",
             "{missing}": "nope.pgm", "{out}": "out.bin"}
    paths = {k: os.path.join(str(tmp), v) for k, v in files.items()}
    open(paths["{pgm}"], "wb").write(b"P5\n32 32\n255\n" + ramp.tobytes())
    open(paths["{ppm}"], "wb").write(b"P6\n32 32\n255\n" + np.stack([ramp, ramp.T, 255 - ramp], axis=2).tobytes())
    open(paths["{small}"], "wb").write(b"P5\n16 24\n255\n" + bytes(16 * 24))            # the wrong-sized side file: 16 wide, 24 high
    open(paths["{notpng}"], "w").write("not an image\n")                                # a text file named .png
    open(paths["{pgmpng}"], "wb").write(b"P5\n32 32\n255\n" + ramp.tobytes())           # a PGM named .png
    return dict(sorted(paths.items(), key=lambda kv: -len(kv[1])))


def answer(binary, args, paths):
    real = list(args)
    for k, v in paths.items():
        real = [a.replace(k, v) for a in real]
    r = subprocess.run([binary, *real], capture_output=True, timeout=120)
    out, err = r.stdout.decode(), r.stderr.decode()
    for k, v in paths.items():
        out, err = out.replace(v, k), err.replace(v, k)
    return {"args": list(args), "status": r.returncode, "stderr": err, "stdout": out}


def test_every_row_gets_the_recorded_answer(cli, tmp_path):
    paths = write_inputs(tmp_path)
    rows = json.load(open(TABLE))
    assert len(rows) >= 150
    wrong = [(row, got) for row in rows for got in [answer(cli, row["args"], paths)] if got != row]
    assert not wrong, "\n".join(f"{row['args']}: expected {row!r}, got {got!r}" for row, got in wrong[:5])
    assert not any("HIP backend" in row["stderr"] for row in rows)                      # no row reaches a device


if __name__ == "__main__":
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        paths = write_inputs(tmp)
        rows = [answer(sys.argv[1], row["args"], paths) for row in json.load(open(TABLE))]
    assert all(row["status"] in (0, 1) for row in rows) and not any("HIP backend" in row["stderr"] for row in rows)
    with open(TABLE, "w") as f:
        json.dump(rows, f, indent=1)
        f.write("\n")
