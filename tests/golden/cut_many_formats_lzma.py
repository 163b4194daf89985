"""How tests/golden/many_formats_16_lzma.bin and many_formats_lzma.json were cut out of the reference's test/many_formats.zip:
    python3 cut_many_formats_lzma.py <path to many_formats.zip>
The payload is copied as it lies in the archive (data, not program text); the size, CRC-32 and flags are the directory's, the SHA-256 is that of
the bytes liblzma decodes from it."""
import hashlib
import json
import lzma
import os
import struct
import sys
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))


def main(path):
    with zipfile.ZipFile(path) as z:
        info = z.getinfo("$16_lzma.tmp")
    assert info.compress_type == 14 and info.flag_bits == 0
    with open(path, "rb") as f:
        f.seek(info.header_offset)
        h = f.read(30)
        assert h[:4] == b"PK\x03\x04"
        nlen, xlen = struct.unpack("<HH", h[26:30])
        f.seek(info.header_offset + 30 + nlen + xlen)
        payload = f.read(info.compress_size)
    d = lzma.LZMADecompressor(lzma.FORMAT_ALONE)
    data = d.decompress(payload[4:9] + info.file_size.to_bytes(8, "little") + payload[9:])
    assert d.eof and len(data) == info.file_size
    with open(os.path.join(HERE, "many_formats_16_lzma.bin"), "wb") as f:
        f.write(payload)
    meta = {"source": "test/many_formats.zip of the reference: the compressed payload of its LZMA entry (data, not program text)",
            "entries": [{"file": "many_formats_16_lzma.bin", "entry": "$16_lzma.tmp", "format": 14, "flags": info.flag_bits, "csize": len(payload),
                         "size": info.file_size, "crc32": "%08x" % info.CRC, "sha256": hashlib.sha256(data).hexdigest()}]}
    with open(os.path.join(HERE, "many_formats_lzma.json"), "w") as f:
        json.dump(meta, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
