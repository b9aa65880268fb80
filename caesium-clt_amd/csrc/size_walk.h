// size_walk.h -- libcaesium's size-targeting as one decision (compress_to_size_in_memory; SURVEY.md 2b [UPSTREAM-RECALL], corroborated by the sample whose
// quantiser scale is the q=51 this walk reaches: 80,40,60,50,55,52,51): bisection on quality from 80 inside (1,101); stop when the result fits and is within 2 %
// of the target, or when the midpoint stops moving (the file of that last try is returned, fitting or not); a walk that bottoms out at q=1 still too large
// returns that smallest file only if return_smallest; more than 10 tries is an error.  Host only, no dependencies: tests/size_walk_check.cpp drives it alone.
#pragma once
#include <cstddef>

struct SizeWalk { int quality = 80, last_less = 1, last_high = 101, tries = 0; bool done = false; };

struct WalkStep {
    enum What { TRY, KEEP, TOO_BIG } what;
    int quality;       // TRY: the quality of the next try
    const char *msg;   // TOO_BIG: which of the two messages
};

// the file of the try at walk.quality came out `length` bytes long: what happens to it next
inline WalkStep step(SizeWalk &w, size_t length, size_t max_output_size, bool return_smallest) {
    const size_t tolerance = max_output_size * 2 / 100;
    if (length <= max_output_size && max_output_size - length < tolerance) return {WalkStep::KEEP, w.quality, nullptr};
    if (length <= max_output_size) w.last_less = w.quality; else w.last_high = w.quality;
    int nq = (w.last_high + w.last_less) / 2;
    nq = nq < 1 ? 1 : (nq > 100 ? 100 : nq);
    if (nq == w.quality) {
        if (nq == 1 && w.last_high == 1 && !return_smallest) return {WalkStep::TOO_BIG, nq, "cannot compress to the requested size"};
        return {WalkStep::KEEP, nq, nullptr};
    }
    // kept as libcaesium states it, though no walk gets here: a bisection inside (1,101) stalls after seven tries at the most
    if (++w.tries >= 10) return {WalkStep::TOO_BIG, nq, "max tries reached while compressing to size"};
    w.quality = nq;
    return {WalkStep::TRY, nq, nullptr};
}
