// Stand-in for <glm/gtx/intersect.hpp>.  The reference includes it (utils.cu) and calls nothing from it: its
// ray / triangle test is its own TriangleHit.
#pragma once
#include "../glm.hpp"
