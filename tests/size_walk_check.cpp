// size_walk_check.cpp -- size_walk.h alone, driven from stdin (tests/test_routes_emul.py builds this with g++ and holds the answers to its own model of the walk).
// One case per line: max_output_size, return_smallest (0 / 1), then the size of the file at every quality 1..100.
// Answer per line: the qualities tried, in order, then "keep <quality>" or "too_big <message>".
#include <cstdio>
#include <vector>

#include "size_walk.h"

int main() {
    for (;;) {
        unsigned long long max_size = 0;
        int return_smallest = 0;
        if (scanf("%llu %d", &max_size, &return_smallest) != 2) return 0;
        std::vector<unsigned long long> size(101, 0);
        for (int q = 1; q <= 100; q++) if (scanf("%llu", &size[q]) != 1) return 2;
        SizeWalk w;
        for (int tries = 0;; tries++) {
            if (tries > 20 || w.quality < 1 || w.quality > 100) { printf("runaway\n"); return 1; }
            printf("%d ", w.quality);
            const int tried = w.quality;
            const WalkStep s = step(w, size_t(size[tried]), size_t(max_size), return_smallest != 0);
            if (s.what == WalkStep::TRY) { if (s.quality != w.quality) { printf("step and walk disagree\n"); return 1; } continue; }
            if (s.what == WalkStep::KEEP) printf("keep %d\n", tried); else printf("too_big %s\n", s.msg);
            break;
        }
    }
}
