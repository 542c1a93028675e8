"""CLI mirror of /root/reference/evaluate.py:  python evaluate.py {pre-calculate|calc} image_path stats_path model_path output_file
The arithmetic is the reference's (fid.py:112-163,185-188) with the activation mean / covariance on the MI355X (lg_fid_stats).
`image_path` names the saved Inception pool_3 activations of the images (an .npy / .npz file, or a directory holding
activations.npy) instead of the JPEGs themselves: the frozen Inception graph the reference downloads (fid.py:276) cannot be
obtained here; `model_path` (where the reference keeps that graph) is accepted and unused.
`calc --metrics fid,kid,prdc` adds KID and precision / recall / density / coverage (littlegan_amd/metrics.py; not in the reference):
they compare against the real images' activations themselves (--real-activations), and log to <output_file>.kid / <output_file>.prdc."""
import argparse

from littlegan_amd import fid
from littlegan_amd.config import metric_list

parser = argparse.ArgumentParser()
parser.add_argument("mode", choices=["pre-calculate", "calc"])
parser.add_argument("image_path")
parser.add_argument("stats_path")
parser.add_argument("model_path")
parser.add_argument("output_file", nargs="?", default=None)
parser.add_argument("--gpu", default="")
parser.add_argument("--chunk-rows", type=int, default=None,
                    help="stream the activations in blocks of this many rows (ActivationAccumulator) instead of loading them whole")
parser.add_argument("--device-sqrt", action="store_true",
                    help="tr sqrt(S1 S2) by the fp64 Newton-Schulz iteration (on the GPU when there is one) instead of scipy's sqrtm")
parser.add_argument("--metrics", default="fid", help="calc: comma list out of fid, kid, prdc")
parser.add_argument("--real-activations", default=None,
                    help="saved activations of the real images: kid and prdc need them (the stats file holds only mu and sigma)")
parser.add_argument("--kid-subsets", type=int, default=100, help="subsets of the KID estimate; 0 = one estimate over the full sets")
parser.add_argument("--kid-subset-size", type=int, default=1000)
parser.add_argument("--prdc-k", type=int, default=3, help="k of the k-NN manifolds of precision / recall / density / coverage")
parser.add_argument("--seed", type=int, default=0, help="seed of the KID subset draws")
args = parser.parse_args()
if args.mode == "pre-calculate":
    fid.pre_calculate(args.image_path, args.stats_path, chunk_rows=args.chunk_rows, device_sqrt=args.device_sqrt)
else:
    if args.output_file is None:
        parser.error("calc needs an output log file")
    try:
        selected = metric_list(args.metrics)
    except ValueError as e:
        parser.error(str(e))
    if set(selected) & {"kid", "prdc"} and args.real_activations is None:
        parser.error("--metrics kid / prdc need --real-activations")
    if "fid" in selected:
        fid.calc(args.image_path, args.stats_path, args.output_file, chunk_rows=args.chunk_rows, device_sqrt=args.device_sqrt)
    if "kid" in selected:
        from littlegan_amd import metrics
        metrics.calc_kid(args.image_path, args.real_activations, args.output_file + ".kid", subsets=args.kid_subsets,
                         subset_size=args.kid_subset_size, seed=args.seed, chunk_rows=args.chunk_rows)
    if "prdc" in selected:
        from littlegan_amd import metrics
        metrics.calc_prdc(args.image_path, args.real_activations, args.output_file + ".prdc", k=args.prdc_k, chunk_rows=args.chunk_rows)
