#!/bin/bash
# LM-fused search, two runs on the same box
echo "search: $(python profiles/tools/time_lm_search.py | tail -1)"
echo "search: $(python profiles/tools/time_lm_search.py | tail -1)"
