#pragma once
// Serial stand-in: no tridiagonal solver is used by the pinned paths.
