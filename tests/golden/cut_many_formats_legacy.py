"""How tests/golden/many_formats_01_pk090.bin .. many_formats_07_pk110.bin and many_formats_legacy.json were cut out of the reference's
test/many_formats.zip:
    python3 cut_many_formats_legacy.py <path to many_formats.zip>
The payloads (PKZIP's own Reduce_1 .. _4, Shrink and Implode streams) are copied as they lie in the archive (data, not program text); the size,
CRC-32, method and flags are the directory's, the SHA-256 is that of the stored entry beside them, which holds the same bytes."""
import hashlib
import json
import os
import struct
import sys
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
ENTRIES = (("$01PK090.TMP", "many_formats_01_pk090.bin"), ("$02PK090.TMP", "many_formats_02_pk090.bin"), ("$03PK090.TMP", "many_formats_03_pk090.bin"),
           ("$04PK090.TMP", "many_formats_04_pk090.bin"), ("$05PK090.TMP", "many_formats_05_pk090.bin"), ("$06PK101.TMP", "many_formats_06_pk101.bin"),
           ("$07PK110.TMP", "many_formats_07_pk110.bin"))


def main(path):
    rows = []
    with zipfile.ZipFile(path) as z:
        plain = z.read("$00store.tmp")
        infos = [z.getinfo(name) for name, _ in ENTRIES]
    with open(path, "rb") as f:
        for info, (name, out) in zip(infos, ENTRIES):
            assert 1 <= info.compress_type <= 6 and info.file_size == len(plain) and info.CRC == infos[0].CRC
            f.seek(info.header_offset)
            h = f.read(30)
            assert h[:4] == b"PK\x03\x04"
            nlen, xlen = struct.unpack("<HH", h[26:30])
            f.seek(info.header_offset + 30 + nlen + xlen)
            payload = f.read(info.compress_size)
            with open(os.path.join(HERE, out), "wb") as g:
                g.write(payload)
            rows.append({"file": out, "entry": name, "format": info.compress_type, "flags": info.flag_bits, "csize": len(payload),
                         "size": info.file_size, "crc32": "%08x" % info.CRC, "sha256": hashlib.sha256(plain).hexdigest()})
    meta = {"source": "test/many_formats.zip of the reference: the compressed payloads of its Reduce, Shrink and Implode entries, written by PKZIP "
                      "0.90 .. 1.10 (data, not program text)", "entries": rows}
    with open(os.path.join(HERE, "many_formats_legacy.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
