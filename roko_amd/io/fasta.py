"""Minimal FASTA reader/writer (the image has no Biopython).

The reference uses Bio.SeqIO for contig parsing and writing
(features.py:125-126, inference.py:149-154); this module provides the same
capability with zero dependencies.
"""

from __future__ import annotations

import gzip
import io
import os
from typing import Iterator, Tuple


def _open_text(path: str):
    if path.endswith(".gz"):
        return io.TextIOWrapper(gzip.open(path, "rb"))
    return open(path, "r")


def read_fasta(path: str) -> Iterator[Tuple[str, str]]:
    """Yield ``(name, sequence)`` per record. Name = header up to first space."""
    name = None
    parts: list[str] = []
    with _open_text(path) as fh:
        for line in fh:
            line = line.rstrip("\n")
            if not line:
                continue
            if line.startswith(">"):
                if name is not None:
                    yield name, "".join(parts)
                name = line[1:].split()[0]
                parts = []
            else:
                if name is None:
                    raise ValueError(f"{path}: sequence data before first header")
                parts.append(line.strip())
    if name is not None:
        yield name, "".join(parts)


def write_fasta(path: str, records, width: int = 80) -> None:
    """Write ``(name, sequence)`` pairs; creates parent dirs."""
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, "w") as fh:
        for name, seq in records:
            fh.write(f">{name}\n")
            for i in range(0, len(seq), width):
                fh.write(seq[i : i + width])
                fh.write("\n")


def write_fastq(path: str, records) -> None:
    """Write ``(name, sequence, quality)`` triples as 4-line FASTQ records,
    unwrapped; `quality` is the Phred+33 string, one char per base. Creates
    parent dirs."""
    d = os.path.dirname(os.path.abspath(path))
    os.makedirs(d, exist_ok=True)
    with open(path, "w") as fh:
        for name, seq, qual in records:
            if len(seq) != len(qual):
                raise ValueError(
                    f"{name}: {len(seq)} bases but {len(qual)} qualities")
            fh.write(f"@{name}\n{seq}\n+\n{qual}\n")


def read_fastq(path: str) -> Iterator[Tuple[str, str, str]]:
    """Yield ``(name, sequence, quality)`` per 4-line record (the form
    `write_fastq` writes). Name = header up to first space."""
    with _open_text(path) as fh:
        while True:
            head = fh.readline()
            if not head:
                return
            head = head.rstrip("\n")
            if not head:
                continue
            seq = fh.readline().rstrip("\n")
            plus = fh.readline().rstrip("\n")
            qual = fh.readline().rstrip("\n")
            if not head.startswith("@") or not plus.startswith("+") \
                    or len(seq) != len(qual):
                raise ValueError(f"{path}: malformed FASTQ record {head!r}")
            yield head[1:].split()[0], seq, qual
