"""Shared helpers: build one named scene on either implementation and render it (through tests/parity.py); the oracle's
golden files; read a built library's kernel metadata."""
import glob
import os
import re
import subprocess
import tempfile

import numpy as np

from rtmi import scenes

_MESH = {}


def small_mesh(n=9):
    if n not in _MESH:
        _MESH[n] = scenes.procedural_bunny_mesh(n)  # 12*n*n triangles (972 by default)
    return _MESH[n]


def build_scene(b, name, aspect=1.0, **kw):
    """Run scene program `name` on builder `b` (oracle's or product's)."""
    if name == "cornell_box":
        scenes.cornell_box(b, aspect)
    elif name == "spheres":
        scenes.spheres(b, aspect)
    elif name == "bunny":
        scenes.bunny(b, aspect, kw.get("faces", small_mesh()), k_min=kw.get("k_min", 2048))
    elif name == "birthday":
        scenes.birthday(b, aspect, kw.get("earthmap", scenes.procedural_earthmap(64, 128)))
    elif name == "sky_only":
        scenes.sky_only(b, aspect)
    elif name == "furnace":
        scenes.furnace(b, aspect, kw.get("rho", 0.5))
    elif name == "mixed":
        scenes.mixed(b, aspect)
    else:
        raise KeyError(name)
    return b


def scene_seed(name):
    return scenes.SCENE_SEEDS.get(name, 1024)


def oracle_render(name, h, w, spp, depth, post=True, seed=None, threads=None, **kw):
    import oraclelib
    import parity
    seed = scene_seed(name) if seed is None else seed
    b = build_scene(oraclelib.OracleBuilder(seed), name, w / h, **kw)
    f = parity.oracle_frame(b, h, w, spp, depth, post, threads)
    return f.image, f.counts, f.states, f.total, b


def gpu_render(name, h, w, spp, depth, post=True, seed=None, world_size=1, **kw):
    """Render through librtmi (C ABI) on cuda:0; world_size > 1 renders every shard on the
    one GPU and assembles them as an RCCL gather would.  The states are the ranks' tile-major planes."""
    import parity
    import rtmi
    seed = scene_seed(name) if seed is None else seed
    b = build_scene(rtmi.SceneBuilder(seed), name, w / h, **kw).commit()
    img, cnt, states, total, _ = parity.render_shards(b, h, w, spp, depth, post, world=world_size)
    return img, cnt, states, total, b


def rel_l2(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    return float(np.sqrt(((a - b) ** 2).sum()) / max(np.sqrt((b ** 2).sum()), 1e-30))


def code_object_notes(lib):
    """One {kernel name: its block of metadata notes (llvm-readelf --notes)} per gfx950 code object embedded in the
    shared library at path `lib`: each translation unit with kernels has a bundle of its own in .hip_fatbin."""
    llvm = "/opt/rocm/lib/llvm/bin"
    assert os.path.exists(llvm + "/llvm-readelf"), "llvm-readelf reads the code object's metadata"
    assert os.path.exists(lib), lib + " missing: __graft_entry__.build() builds it"
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fatbin")
        subprocess.check_call([llvm + "/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib, fat])
        data = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(b"__CLANG_OFFLOAD_BUNDLE__", data)]
        for k, at in enumerate(starts):
            part, co = os.path.join(tmp, "part%d" % k), os.path.join(tmp, "co%d.o" % k)
            with open(part, "wb") as f:
                f.write(data[at:starts[k + 1] if k + 1 < len(starts) else len(data)])
            subprocess.check_call([llvm + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + part,
                                   "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co], stderr=subprocess.DEVNULL)
            notes = subprocess.check_output([llvm + "/llvm-readelf", "--notes", co], text=True)
            out.append({re.search(r"\.name:\s+(\S+)", blk).group(1): blk for blk in notes.split("- .agpr_count")[1:]})
    return out


def kernel_notes(lib):
    """Kernel name -> its block of metadata notes, over every gfx950 code object of the shared library at path `lib`."""
    return {name: blk for notes in code_object_notes(lib) for name, blk in notes.items()}


HERE = os.path.dirname(os.path.abspath(__file__))
# the oracle's own goldens; ref_*.npz, the reference renderer's records, are read by test_ref_golden.py
FILES = sorted(f for f in glob.glob(os.path.join(HERE, "golden", "*.npz")) if not os.path.basename(f).startswith("ref_"))
PAT = re.compile(r"(?P<name>[a-z_]+)_(?P<h>\d+)x(?P<w>\d+)_s(?P<spp>\d+)_d(?P<depth>\d+)_(?P<mode>post|raw)\.npz$")


def parse_case(path):
    m = PAT.search(os.path.basename(path))
    assert m, path
    kw = {"k_min": 64} if m["name"] == "bunny" else {}
    return m["name"], int(m["h"]), int(m["w"]), int(m["spp"]), int(m["depth"]), m["mode"] == "post", kw
