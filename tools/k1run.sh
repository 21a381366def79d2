O=${OUT_DIR:?set OUT_DIR to the folder the results go to}
mkdir -p "$O"
for lib in libflakehip.so libflakehip_noprod.so libflakehip_nowalk.so; do for sp in 0 1; do
# the probe libraries: `python -m flake_amd.build probes` (built before the run); a missing one is skipped
if [ $sp = 0 ]; then export FHIP_NO_LAG_SPLIT=1; else unset FHIP_NO_LAG_SPLIT; fi
FHIP_LIB=$PWD/flake_amd/lib/$lib python bench.py --full --frames 512 --no-cpu-baseline --no-other-configs --steps 200 --warmup 50 > $O/r03_k1p.json 2> $O/r03_k1p.err
python -c "
import json;d=json.load(open('$O/r03_k1p.json'));print('$lib split=$sp',d['ms_per_step'],d['roofline']['kernel_ms'])" || tail -3 $O/r03_k1p.err
done; done
