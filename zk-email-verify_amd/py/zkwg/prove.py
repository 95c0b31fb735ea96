"""python -m zkwg.prove circuit.zkey witness.wtns proof.json public.json -- `snarkjs groth16 prove` on the device (reference call site:
snarkjs.groth16.fullProve = wtns.calculate + groth16.prove, packages/helpers/src/chunked-zkey.ts:80-84)."""
import argparse
import json
import secrets
import sys

from .prover import Prover, WitnessProver, R


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("zkey")
    ap.add_argument("wtns")
    ap.add_argument("proof_json")
    ap.add_argument("public_json")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    wp = WitnessProver(open(a.zkey, "rb").read(), device=a.device, slots=1)
    w = open(a.wtns, "rb").read()
    st, proofs = wp.prove([w], [(secrets.randbelow(R), secrets.randbelow(R))])
    if st[0] != 0:
        print(f"no proof: {wp.lib.zkwg_strerror(st[0]).decode()}", file=sys.stderr)
        return 1
    json.dump(Prover.proof_json(proofs[0]), open(a.proof_json, "w"), indent=1)
    json.dump(wp.public_signals(w), open(a.public_json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
