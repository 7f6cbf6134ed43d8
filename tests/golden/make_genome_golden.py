#!/usr/bin/env python3
"""Records tests/golden/genome/: a few small FASTA genomes and beside each the .ann, .amb and .pac the reference writes for it
(Pack::vAppendFASTA + vStoreCollection, through `oracle/_ref/ref_dump fastapack <fa> <prefix>`).  tests/test_genome_text_host.py
holds ma_genome_dev::parseHost to them: contig names, starts, lengths and holes per contig (.ann), the holes (.amb) and the 2-bit
bases outside the holes (.pac; inside them the reference draws from a generator it seeds with the time).  Between them the files
have multi-line contigs of unequal line lengths, a last line without a line feed, "\\r\\n" line ends, lower case, a header with a
comment, runs of N at a contig's start and end with the next contig starting in N, a run across a line end, R and Y inside a run
of N, and a single N.
Run:  python tests/golden/make_genome_golden.py"""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))

FILES = {
    # holes at 0+2, 10+6, 24+1, 25+1, 46+26 of the forward strand
    "mixed.fa": b">c1 first contig\nNNACGTacgtNN\nNNRYACGT\nACGTN\n>c2\nNACGTTTGACCATGACCAGTC\nN\nNNNNNNNNNNNNNNNNNNNNNNNNN\n"
                b">c3\nacgtacgtacgtaNcgtacgtacgatcgatcgatcgatcgactagctagctagcatcgatcgatcagctagctagcta\nGGA\nTTTTTCAGCGACGAGCAGCGACGGAG",
    "crlf.fa": b">one\r\nACGTNNAC\r\nNNNNGT\r\nA\r\n>two words here\r\nnnnnACGTGGTCAGTCGATGACGTACGTACGTAGCTNNNN\r\nNNAACC\r\n",
    "plain.fa": b">chrA\nACGTACGGTCAGTCGATCGATCGACTAGCATCGATCGACTAGCTAGCATCGACTAGCTAGCTAGCATCGAT\nACGGT\n>chrA\nGGGGACTAGCTAC\n>chrB 2\nTTGACN\n"
                b"ACGACTGACTAGCTAGCTAGCATCGATCGATCAGCTAGCTACGAT\n",
}

if __name__ == "__main__":
    out = os.path.join(HERE, "genome")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(ROOT, "oracle", "_ref", "ref_dump")
    for name, data in FILES.items():
        fa = os.path.join(out, name)
        with open(fa, "wb") as f:
            f.write(data)
        subprocess.check_call([exe, "fastapack", fa, fa[:-3]])
