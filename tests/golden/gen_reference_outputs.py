"""Builds tests/golden/reference_outputs.npz from DATA files of the reference's sample outputs (`output_imgs/{indoor,jinjya}`, run in the
build container only).  Only pixels and file bytes are stored, no reference code.  Used by tests/test_reference_outputs.py.

  * `{scene}_{name}_exr`: a valid PIZ-compressed OpenEXR file made of one of the shipped file's own 32-line chunks (rows 192-223, bytes
    unchanged; header dataWindow and offset table rewritten for it) -- the input of the PIZ decoder under test; rows chosen so that
    the roughness band holds both clamp values of the loop (0.07 and 1.0).
  * `{scene}_panel_u8`: the same rows of `opt_env_img.png` (8-bit RGB as PIL decodes it): the independent encoding of the same pictures.
  * `indoor_render_*`: eight bands of 4 rows spread over the image (`RENDER_ROWS`) of the optimised maps and of Mitsuba's render of them;
    `indoor_depth_rows` the depth rows of those bands and one row above and below each (what central differences read), `indoor_depth_max`
    the image's maximum depth (the flip of inverse_img_w_mi.py:722 uses it), `indoor_envmap` the optimised envmap texels.
"""
import os
import struct
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from materialist_amd.imageio_exr import read_exr  # noqa: E402
from materialist_amd.imageio_hdr import read_hdr  # noqa: E402

OUT = "/root/reference/output_imgs"
PIZ_CHUNKS = (6,)              # 32-line chunks: rows 192-223
RENDER_ROWS = [r for k in range(8) for r in range(30 + 64 * k, 34 + 64 * k)]


def exr_chunks(path: str, chunks) -> bytes:
    """The EXR file at `path` cut down to the given consecutive 32-line chunks (PIZ), chunk bytes unchanged."""
    data = open(path, "rb").read()
    pos, attrs = 8, {}
    while data[pos] != 0:
        end = data.index(b"\0", pos)
        name = data[pos:end].decode()
        end2 = data.index(b"\0", end + 1)
        (size,) = struct.unpack_from("<i", data, end2 + 1)
        attrs[name] = (pos, end2 + 5, size)
        pos = end2 + 5 + size
    header_end = pos + 1
    assert data[attrs["compression"][1]] == 4, "PIZ expected"
    x0, y0, x1, y1 = struct.unpack_from("<iiii", data, attrs["dataWindow"][1])
    nblocks = (y1 - y0 + 32) // 32
    offsets = struct.unpack_from(f"<{nblocks}Q", data, header_end)
    blobs = []
    for c in chunks:
        y, size = struct.unpack_from("<ii", data, offsets[c])
        assert y == y0 + 32 * c
        blobs.append(data[offsets[c]: offsets[c] + 8 + size])
    head = bytearray(data[:header_end])
    struct.pack_into("<iiii", head, attrs["dataWindow"][1], x0, y0 + 32 * chunks[0], x1, y0 + 32 * chunks[-1] + 31)
    table, off = [], header_end + 8 * len(chunks)
    for b in blobs:
        table.append(off)
        off += len(b)
    return bytes(head) + struct.pack(f"<{len(chunks)}Q", *table) + b"".join(blobs)


def main():
    rows = slice(32 * PIZ_CHUNKS[0], 32 * PIZ_CHUNKS[-1] + 32)
    d = {"piz_rows": np.array([rows.start, rows.stop], np.int32), "render_rows": np.array(RENDER_ROWS, np.int32)}
    for scene in ("indoor", "jinjya"):
        names = {"roughness": "best_results/roughness.exr", "gt": "gt_image.exr"}
        if scene == "indoor":
            names["render"] = "best_results/rendered_img.exr"
        for k, f in names.items():
            b = exr_chunks(f"{OUT}/{scene}/{f}", PIZ_CHUNKS)
            assert np.array_equal(read_exr_bytes(b), read_exr(f"{OUT}/{scene}/{f}")[rows])
            d[f"{scene}_{k}_exr"] = np.frombuffer(b, np.uint8)
        panel = np.asarray(Image.open(f"{OUT}/{scene}/opt_env_img.png").convert("RGB"))
        d[f"{scene}_panel_u8"] = panel[rows, : 1024 if scene == "indoor" else 512].copy()       # the columns the test reads
    ind = f"{OUT}/indoor"
    for k in ("albedo", "roughness", "metallic", "rendered_img"):
        d[f"indoor_render_{k}"] = read_exr(f"{ind}/best_results/{k}.exr")[RENDER_ROWS]
    depth = read_exr(f"{ind}/depthPred.exr")[..., 0]
    near = sorted({i + o for i in RENDER_ROWS for o in (-1, 0, 1) if 0 <= i + o < depth.shape[0]})
    d["indoor_depth_row_index"] = np.array(near, np.int32)
    d["indoor_depth_rows"] = depth[near]
    d["indoor_depth_max"] = np.float32(depth.max())
    d["indoor_image_hw"] = np.array(depth.shape, np.int32)
    d["indoor_envmap"] = read_hdr(f"{ind}/best_results/envmap.hdr").astype(np.float32)
    np.savez_compressed(os.path.join(HERE, "reference_outputs.npz"), **d)
    print({k: (v.shape, str(v.dtype)) for k, v in d.items()})


def read_exr_bytes(b: bytes) -> np.ndarray:
    import tempfile

    with tempfile.NamedTemporaryFile(suffix=".exr") as f:
        f.write(b)
        f.flush()
        return read_exr(f.name)


if __name__ == "__main__":
    main()
