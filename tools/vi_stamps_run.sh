set -o pipefail
cd "$GRAFT_REPO_ROOT" 2>/dev/null || cd /root/repo
mkdir -p bench_out/vist
MGCM_LIB=mitgcm_amd/_build/diag/libmitgcm_amd_vistamps.so timeout -k 10 200 python bench.py --full --config llc90_synthetic --steps 2 --warmup 1 --no-cpu-baseline > bench_out/vist/out.txt 2> bench_out/vist/err.txt || { tail -5 bench_out/vist/err.txt; exit 1; }
grep -c VISTAMP bench_out/vist/out.txt
