#!/usr/bin/env python3
"""Generate tests/golden/crop_grid.json by running the REFERENCE's own tools/crop_img.sh under bash (build container only).

Run:  python tests/golden/make_golden_crop_grid.py      (needs bash and the reference checkout make_golden.py names)

The script is executed as it stands, never copied.  Three stand-in programs come first on PATH, because the real ones
(ImageMagick, jpegtran, file) are absent here and no image exists:
  file       prints "<path>: PNG image data, <W> x <H>, 8-bit/color RGB, non-interlaced" with the size of the case (from the
             environment), which is the text the script's grep takes the size from
  convert    appends its arguments, one line per call, to the record file of the case; writes nothing else
  jpegtran   the same, for the .jpg case
What is stored is what the script asked of them: for each (W, H, cs, stride) the -crop geometry and the output file name of every
call, in the order of the calls.

Layout: a JSON list of {"width", "height", "cs", "stride", "ext", "basename", "crops": [{"geometry": "<w>x<h>+<x>+<y>",
"name": "<basename>_<xcrop>_<ycrop>_<useful size>.<ext>"}, ...]}.
"""
import json
import os
import stat
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import REF  # noqa: E402  (where the reference lives)

SCRIPT = os.path.join(REF, "tools", "crop_img.sh")
BASENAME = "NIND_scene_ISO200"
# width, height, cs, stride, ext
CASES = [
    (812, 620, 128, 96, "png"),
    (768, 620, 128, 96, "png"),        # a width divisible by the stride: the case the script's own TODO worries about
    (812, 576, 128, 96, "png"),        # and a height
    (6000, 4000, 256, 192, "png"),
    (300, 200, 256, 192, "png"),       # no crop
    (256 + 32, 256 + 32, 256, 192, "png"),     # both sides exactly cs + (cs - stride) / 2: one crop
    (256 + 31, 400, 256, 192, "png"),          # one pixel short of it: none
    (128 + 16, 500, 128, 96, "png"),           # a width of exactly cs + (cs - stride) / 2
    (404, 500, 128, 96, "png"),
    (528, 400, 176, 128, "png"),
    (384, 384, 128, 128, "png"),       # cs == stride: no margin, the first column and row are full crops
    (400, 300, 128, 128, "png"),
    (812, 620, 128, 96, "jpg"),        # the jpegtran branch issues the same geometries
    (240, 160, 64, 8, "tif"),          # a wide margin: (cs - stride) / 2 = 28
]

FILE_STUB = """#!/bin/sh
echo "$1: PNG image data, ${GRID_W} x ${GRID_H}, 8-bit/color RGB, non-interlaced"
"""
RECORD_STUB = """#!/bin/sh
echo "$@" >> "${GRID_RECORD}"
"""


def run_case(bindir, workdir, width, height, cs, stride, ext):
    record = os.path.join(workdir, "record.txt")
    if os.path.exists(record):
        os.remove(record)
    outdir = os.path.join(workdir, "out")
    fpath = os.path.join(workdir, f"{BASENAME}.{ext}")
    env = dict(os.environ, PATH=bindir + os.pathsep + os.environ["PATH"], GRID_W=str(width), GRID_H=str(height), GRID_RECORD=record)
    subprocess.run(["bash", SCRIPT, str(cs), str(stride), fpath, outdir], check=True, env=env, stdout=subprocess.DEVNULL)
    crops = []
    if os.path.exists(record):
        with open(record) as f:
            for line in f:
                words = line.split()
                geometry = words[words.index("-crop") + 1]
                # convert -crop G <in> <out>; jpegtran -crop G -copy none -optimize -outfile <out> <in>
                out = words[words.index("-outfile") + 1] if "-outfile" in words else words[-1]
                assert os.path.dirname(out) == outdir and fpath in words, line
                crops.append({"geometry": geometry, "name": os.path.basename(out)})
    return {"width": width, "height": height, "cs": cs, "stride": stride, "ext": ext, "basename": BASENAME, "crops": crops}


def main():
    with tempfile.TemporaryDirectory() as tmp:
        bindir = os.path.join(tmp, "bin")
        os.makedirs(bindir)
        for name, text in (("file", FILE_STUB), ("convert", RECORD_STUB), ("jpegtran", RECORD_STUB)):
            path = os.path.join(bindir, name)
            with open(path, "w") as f:
                f.write(text)
            os.chmod(path, os.stat(path).st_mode | stat.S_IXUSR)
        cases = [run_case(bindir, tmp, *case) for case in CASES]
    out = os.path.join(HERE, "crop_grid.json")
    with open(out, "w") as f:
        json.dump(cases, f, indent=1)
        f.write("\n")
    for c in cases:
        print(f"{c['width']} x {c['height']} at {c['cs']}/{c['stride']} .{c['ext']}: {len(c['crops'])} crops")
    print(f"wrote {out} ({os.path.getsize(out)} bytes)")


if __name__ == "__main__":
    main()
