# Build measurement variants of libtrivy_secret.so: the same sources with an instrument
# compiled in (select one with TSG_LIB_VARIANT=<name>).  Every variant computes the same
# results.  (The variants of experiments that did not ship -- other unroll factors, queue
# depths, reserve chunks, ... -- are no longer in the source: DESIGN.md section 5 and the
# profiles/ directories it cites hold their timings.)
#   usage: tools/build_variants.sh NAME...
set -e
cd "$(dirname "$0")/.."
python -m trivy_amd.build
build() {
  name=$1; shift
  mkdir -p /tmp/tsgv_$name
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -x hip -O3 -std=c++17 -fPIC -Wall -Wno-unused-function "$@" -Iinclude \
    -c trivy_amd/csrc/kernels.hip -o /tmp/tsgv_$name/kernels.o
  objs=$(ls trivy_amd/build/*.o | grep -v kernels.hip.o)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o trivy_amd/libtrivy_secret_$name.so $objs /tmp/tsgv_$name/kernels.o -lpthread
}
for v in "$@"; do
  case $v in
    k2ctr) build $v -DK2_TRACE_CTR ;;      # K2: per-entry counters (TSG_K2_TRACE, tools/k2trace.py)
    k2phase) build $v -DK2_TRACE_PHASE ;;  # K2: per-entry phase stamps of thread 0 (TSG_K2_TRACE)
    xdiag) build $v -DK1X_DIAG ;;          # K1X: verify counters in k2_long_tails (slot probes),
                                           # k2_tail_bytes (entries examined), k2_tail_max (matches)
    ftr) build $v -DK1F_WTRACE=1 ;;        # K1F: per-wave trace (TSG_K1F_TRACE, tools/k1ftrace.py)
    ftr0) build $v -DK1F_WTRACE=1 -DK1F_SHARES=0 ;;  # the same with equal wave ranges
    fe) build $v -DK1F_SHARES=0 ;;         # K1F: equal wave ranges (to re-derive the shares)
    *) echo "unknown variant: $v (k2ctr k2phase xdiag ftr ftr0 fe)" >&2; exit 1 ;;
  esac
done
