for o in 0 1 2 3; do
  line=$(CMH_GEMM_ORDER=$o timeout -k 10 300 python bench.py --steps 10 --warmup 3 --full --no-cpu-baseline --no-map-eval 2>/dev/null | tail -1)
  echo "order=$o $(echo "$line" | grep -o '"value": [0-9.]*') $(echo "$line" | grep -o '"achieved": [0-9.]*')"
done
