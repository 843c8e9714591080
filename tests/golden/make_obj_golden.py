"""Generates tests/golden/obj_golden.npz: the reference-side pin of dgs_amd.io.read_mesh_obj.

The reference's ground-truth reader (read_gt_mesh.py: load_obj, which render_mesh.py imports) runs on a triangle-only OBJ that this
script writes itself: `v` lines with three and with four numbers, `f` lines with plain, `i/t`, `i//n` and `i/t/n` corner tokens,
and the lines it skips (comments, vt, vn, o, g, s, usemtl, blank).  Stored, as arrays only: the bytes of that file, and the
vertices and faces load_obj returned.  The two documented extensions of read_mesh_obj (polygons, negative indices) are outside
the rules shared with the reference and are tested in tests/test_mesh_metrics_cpu.py alone.  Run from the repo root:
    python tests/golden/make_obj_golden.py
"""
import importlib.util
import os
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
SEED, NV, NF = 5, 23, 31


def obj_text():
    g = np.random.default_rng(SEED)
    verts = np.round(g.uniform(-2, 2, (NV, 3)), 6)
    faces = np.stack([g.permutation(NV)[:3] for _ in range(NF)]) + 1
    lines = ["# triangle-only mesh for the OBJ golden", "mtllib none.mtl", "o golden", ""]
    for i, v in enumerate(verts):
        if i % 5 == 0:
            lines.append("v %.6f %.6f %.6f 1.0" % tuple(v))          # a fourth number (w) is ignored
        elif i % 5 == 1:
            lines.append("v  %e\t%e %e" % tuple(v))                   # any whitespace, exponent notation
        else:
            lines.append("v %r %r %r" % tuple(float(x) for x in v))
    lines += ["vt 0.25 0.75", "vt 0.5 0.5", "vn 0 0 1", "g part", "usemtl none", "s off"]
    for i, f in enumerate(faces):
        fmt = ["%d %d %d", "%d/1 %d/2 %d/1", "%d//1 %d//1 %d//1", "%d/2/1 %d/1/1 %d/2/1"][i % 4]
        lines.append("f " + fmt % tuple(f))
        if i == 7:
            lines.append("# a comment between faces")
    return "\n".join(lines) + "\n"


def main():
    spec = importlib.util.spec_from_file_location("ref_read_gt_mesh", os.path.join(REF, "read_gt_mesh.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    text = obj_text().encode("ascii")
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "golden.obj")
        with open(path, "wb") as f:
            f.write(text)
        verts, faces = m.load_obj(path)
    assert verts.shape == (NV, 3) and faces.shape == (NF, 3)
    np.savez_compressed(os.path.join(HERE, "obj_golden.npz"), obj_text=np.frombuffer(text, np.uint8), vertices=np.asarray(verts, np.float64),
                        faces=np.asarray(faces, np.int32))
    print("vertices", verts.shape, verts.dtype, "faces", faces.shape, faces.dtype, "bytes", len(text))


if __name__ == "__main__":
    main()
